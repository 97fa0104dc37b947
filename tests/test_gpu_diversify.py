"""msr_diversify (diversify_kernel, DESIGN K6b) through the raw ABI against the oracle of tests/diversify_cases.py, every
comparison exact: all five outputs of every query (out_doc, out_chunk and out_n as int32, out_score and out_orig as float64 bit
patterns), the padding through max_cand, and a sentinel row behind the call's rows.  fused_orig and fused_chunk carry values
that are distinct per slot and unrelated to the document, so a row assembled from two slots shows.  The exhaustive small lists
of one top_k go into ONE call (thousands of workgroups): that is the multi-query test as well."""
import ctypes as C

import numpy as np
import pytest
import torch

import diversify_cases as dc
from msretr import _abi
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex

pytestmark = pytest.mark.gpu
FILL = -1515870811                                           # 0xA5A5A5A5 as int32
FILL64 = -7.5
INVALID = -1
BEYOND_DOC, BEYOND_SCORE = 7 * dc.SLOTS + 1000, 2.0          # what stands behind fused_n: an accepted, high-scoring entry


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Batch:
    """The [Q, M] inputs of a list of cases: doc and score from the case (BEYOND_* behind it), orig and chunk distinct per slot."""

    def __init__(self, cases, M):
        Q = len(cases)
        self.cases, self.M, self.Q = cases, M, Q
        self.doc = np.full((Q, M), BEYOND_DOC, np.int32)
        self.score = np.full((Q, M), BEYOND_SCORE)
        self.n = np.zeros(Q, np.int32)
        for q, c in enumerate(cases):
            k = min(len(c["doc"]), M)
            self.doc[q, :k], self.score[q, :k] = c["doc"][:k], c["score"][:k]
            self.n[q] = c.get("n", len(c["doc"]))
        slot = np.arange(Q * M, dtype=np.int64).reshape(Q, M)
        self.orig = 0.25 + slot * 0.5
        self.chunk = (1_000_003 + slot * 7).astype(np.int32)

    def arrays(self, lists):
        """lists[q] = [(slot, score)] -> the five outputs as the call pads them."""
        Q, M = self.Q, self.M
        o_doc, o_chunk = np.full((Q, M), -1, np.int32), np.full((Q, M), -1, np.int32)
        o_score, o_orig, o_n = np.full((Q, M), -np.inf), np.zeros((Q, M)), np.zeros(Q, np.int32)
        for q, lst in enumerate(lists):
            k = len(lst)
            o_n[q] = k
            if k:
                s = np.fromiter((i for i, _ in lst), np.int64, k)
                o_doc[q, :k], o_chunk[q, :k], o_orig[q, :k] = self.doc[q, s], self.chunk[q, s], self.orig[q, s]
                o_score[q, :k] = [x for _, x in lst]
        return o_doc, o_score, o_orig, o_chunk, o_n

    def want(self, top_k, thr=dc.T, div=True, table=dc.DOMAIN_TABLE):
        return self.arrays([dc.expected(c, top_k, thr, div, table, self.M) for c in self.cases])


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = CorpusIndex(doc_ids=np.arange(100, dtype=np.int64), doc_off=np.arange(101, dtype=np.int32), chunk_ids=np.arange(100, dtype=np.int64),
                     emb=np.eye(768, dtype=np.float32)[np.arange(100) % 768], total_docs=100)
    e = DeviceEngine(ix, max_queries=8, max_k=100, rerank_max_docs=1000)
    e.bind_doc_domains(dc.DOMAIN_TABLE)
    yield e
    e.close()


def _outs(dev, Q, M):
    i32 = lambda *s: torch.full(s, FILL, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.full(s, FILL64, dtype=torch.float64, device=dev)
    return [i32(Q + 1, M), f64(Q + 1, M), f64(Q + 1, M), i32(Q + 1, M), i32(Q + 1)]


def run(eng, b, top_k, thr=dc.T, div=True):
    """One msr_diversify call into buffers with one query row more than the call writes -> the host arrays."""
    dev = eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [up(b.doc), up(b.score), up(b.orig), up(b.chunk), up(b.n)]
    outs = _outs(dev, b.Q, b.M)
    rc = eng.lib.msr_diversify(eng.handle, b.Q, *map(_P, ins), b.M, int(top_k), C.c_double(thr), 1 if div else 0, *map(_P, outs),
                               eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return [o.cpu().numpy() for o in outs]


def same(got, want, b, what):
    Q = b.Q
    for g, w, name in zip(got, want, ("doc", "score", "orig", "chunk", "n")):
        gq, wq = (_bits(g[:Q]), _bits(w)) if g.dtype == np.float64 else (g[:Q], w)
        bad = np.argwhere(gq != wq)
        if len(bad):
            q = int(bad[0][0])
            c = b.cases[q]
            raise AssertionError((what, name, bad[:4].tolist(), c["name"], c["doc"][:12].tolist(), c["score"][:12].tolist(),
                                  np.atleast_1d(g[q])[:12].tolist(), np.atleast_1d(w[q])[:12].tolist()))
        assert (g[Q] == (FILL64 if g.dtype == np.float64 else FILL)).all(), (what, name, "the row behind the call")
    # the padding, stated once more directly: -1 / -inf / 0.0 / -1 from out_n through max_cand
    pad = np.arange(b.M)[None, :] >= got[4][:Q, None]
    assert (got[0][:Q][pad] == -1).all() and np.isneginf(got[1][:Q][pad]).all() and (_bits(got[2][:Q])[pad] == 0).all()
    assert (got[3][:Q][pad] == -1).all()


# ---- exhaustive small lists: one call per top_k and threshold ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    by_k = {}
    for c in dc.small_lists():
        by_k.setdefault(c["top_k"], []).append(c)
    return {k: Batch(v, 8) for k, v in sorted(by_k.items())}


@pytest.mark.parametrize("thr", dc.THRESHOLDS)
def test_every_small_list(eng, small, thr):
    total = 0
    for top_k, b in small.items():
        if thr != dc.T:                                      # the other thresholds: lengths 1 .. 4
            b = Batch([c for c in b.cases if len(c["doc"]) <= 4], 8)
            if not b.Q:
                continue
        assert b.Q > 1000                                    # thousands of workgroups per call: blockIdx.x > 0 against the oracle
        same(run(eng, b, top_k, thr), b.want(top_k, thr), b, ("small", top_k, thr))
        total += b.Q
    assert total == (len(dc.small_lists()) if thr == dc.T else len(dc.small_lists(4)))


def test_every_small_list_with_diversification_off(eng, small):
    for top_k, b in small.items():
        same(run(eng, b, top_k, div=False), b.want(top_k, div=False), b, ("small, off", top_k))


# ---- the named edges, at the two widths that hold them ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    cases = dc.edge_lists()
    return {M: Batch(cases, M) for M in (1000, 1024)}


@pytest.mark.parametrize("M", [1000, 1024])
def test_edge_lists(eng, edges, M):
    b = edges[M]
    assert max(len(c["doc"]) for c in b.cases) == 1024 and (b.n > 1000).sum() >= 5          # at 1000 the long lists are clamped
    for top_k in sorted({c["top_k"] for c in b.cases}):      # every list at every list's top_k
        for thr in (dc.THRESHOLDS if top_k in (5, 1000) else (dc.T,)):
            same(run(eng, b, top_k, thr), b.want(top_k, thr), b, ("edges", M, top_k, thr))
    for top_k in (5, 100, 5000):
        same(run(eng, b, top_k, div=False), b.want(top_k, div=False), b, ("edges, off", M, top_k))


def test_widths(eng):
    seen = set()
    for M, top_k, cases in dc.widths():
        b = Batch(cases, M)
        assert b.n.tolist() == [-3, 0, 1, M - 1, M, M + 7]
        got = run(eng, b, top_k)
        same(got, b.want(top_k), b, ("width", M, top_k))
        assert got[4][:2].tolist() == [0, 0] and (got[4][4] == got[4][5])                 # fused_n below 0 and above max_cand clamp
        same(run(eng, b, top_k, div=False), b.want(top_k, div=False), b, ("width, off", M, top_k))
        seen.add(M)
    assert seen == {1, 2, 63, 64, 65, 1000, 1024}


# ---- the domain table -----------------------------------------------------------------------------------------------------------------
def test_domain_tables(eng, edges):
    """Bound; not bound (every document its own domain, a document index of -1 inside fused_n is rejected and nothing else
    is); shorter than the largest document index (indices at or past its end are rejected: the present, documented
    behaviour); bound and unbound again (the bytes of the unbound call)."""
    cases = [dict(c) for c in edges[1024].cases]
    for c in cases[::3]:                                     # a -1 inside fused_n in every third list
        c["doc"] = c["doc"].copy()
        c["doc"][len(c["doc"]) // 2] = -1
    b = Batch(cases, 1024)
    short = dc.DOMAIN_TABLE[:3 * dc.SLOTS + 2]               # domains 0, 1, 2 and two documents of domain 3
    assert max(int(c["doc"].max()) for c in cases) > len(short) > min(int(c["doc"][c["doc"] >= 0].min()) for c in cases)
    try:
        bound = run(eng, b, 5)
        same(bound, b.want(5), b, "bound")
        assert all((x == y).all() for x, y in zip(run(eng, b, 5), bound))                # a repeated call, equal bytes
        eng.bind_doc_domains(None)
        free = run(eng, b, 5)
        same(free, b.want(5, table=None), b, "no table")
        assert not all((x == y).all() for x, y in zip(free, bound))
        same(run(eng, b, 1000), b.want(1000, table=None), b, "no table, top_k 1000")
        eng.bind_doc_domains(short)
        cut = run(eng, b, 5)
        same(cut, b.want(5, table=short), b, "short table")
        assert not all((x == y).all() for x, y in zip(cut, bound))
        for q, c in enumerate(cases):                        # nothing at or past the table's end is returned
            assert (cut[0][q, :cut[4][q]] < len(short)).all(), c["name"]
        same(run(eng, b, 1000, div=False), b.want(1000, div=False, table=short), b, "short table, off")
        eng.bind_doc_domains(dc.DOMAIN_TABLE)
        eng.bind_doc_domains(None)
        assert all((x == y).all() for x, y in zip(run(eng, b, 5), free))                  # bound and unbound again
    finally:
        eng.bind_doc_domains(dc.DOMAIN_TABLE)
    assert all((x == y).all() for x, y in zip(run(eng, b, 5), bound))


# ---- the engine method ----------------------------------------------------------------------------------------------------------------
def test_engine_method_on_non_contiguous_inputs(eng, edges):
    b = edges[1000]
    dev = eng.device
    wide = lambda a: torch.from_numpy(np.repeat(a, 2, axis=1)).to(dev)[:, ::2]            # every second column of a [Q, 2 M] tensor
    fused = (wide(b.doc), wide(b.score), wide(b.orig), wide(b.chunk), torch.from_numpy(np.repeat(b.n, 3)).to(dev)[::3])
    assert not any(t.is_contiguous() for t in fused)
    for top_k, thr, div in ((5, dc.T, True), (1000, 0.0, True), (30, dc.T, False)):
        raw = run(eng, b, top_k, thr, div)
        got = [x.cpu().numpy() for x in eng.diversify(fused, top_k=top_k, relevance_threshold=thr, diversification=div)]
        assert all(g.shape == r[:b.Q].shape for g, r in zip(got, raw))
        for g, r, name in zip(got, raw, ("doc", "score", "orig", "chunk", "n")):
            assert (_bits(g) == _bits(r[:b.Q])).all() if g.dtype == np.float64 else (g == r[:b.Q]).all(), (name, top_k, thr, div)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(eng, edges):
    dev = eng.device
    b = Batch(edges[1024].cases[:3], 1024)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [up(b.doc), up(b.score), up(b.orig), up(b.chunk), up(b.n)]
    outs = _outs(dev, b.Q, b.M)

    def call(q=b.Q, m=b.M, top_k=5, ins=ins, outs=outs):
        return eng.lib.msr_diversify(eng.handle, q, *map(_P, ins), m, top_k, C.c_double(dc.T), 1, *map(_P, outs), eng._stream())

    def refused(**kw):
        assert call(**kw) == INVALID, kw
        msg = eng.lib.msr_last_error(eng.handle)
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert "msr_diversify" in msg, (kw, msg)

    for k in range(5):
        refused(ins=ins[:k] + [None] + ins[k + 1:])
        refused(outs=outs[:k] + [None] + outs[k + 1:])
    for kw in (dict(m=0), dict(m=1025), dict(top_k=0), dict(q=-1), dict(m=-1), dict(top_k=-5)):
        refused(**kw)
    assert call(q=0) == 0                                    # nothing to do is a success, and launches nothing
    torch.cuda.synchronize(dev)
    assert all((o == (FILL64 if o.dtype == torch.float64 else FILL)).all() for o in outs)
    with pytest.raises(_abi.MsrError):
        eng.diversify(tuple(ins), top_k=0)
    assert call() == 0                                       # ... and the same buffers are fine for a good call
    torch.cuda.synchronize(dev)
    same([o.cpu().numpy() for o in outs], b.want(5), b, "after the refusals")
