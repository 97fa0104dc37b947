"""The exact top-k select (sel_hist / sel_scan / sel_compact / sel_final of msr_topk.hip) on raw score rows, and the list merges
behind msr_merge_topk_payload.  Every case of tests/select_cases.py goes through DeviceEngine.debug_select (msr_debug_select:
the engine's own scratch and kernels) and must equal the plain stable sort exactly: out_n, the documents in order, the score
bits, -1 / -inf behind out_n.  Zeros: -0.0 and +0.0 are one key and come back as +0.0, so an expected zero is compared by
value with +0.0 bits, everything else by bits.  No case is skipped: each one also asserts, from the SelState the call
exports, that every query took the path the CPU model of the control flow predicts (all eight fields, exactly), and that the
branches the case is built for are among them.  Every case runs twice in a row (the select's scratch must be all zero between
calls), every large-tie case is followed by a small ordinary one on the same engine.

Not here: a cross-check against msr_dense_topk's own score rows -- they live in engine scratch no entry point exposes.  The
BM25 cross-check rebuilds the candidate row from msr_bm25_score_docs, whose scores are msr_bm25_topk's bit for bit."""
import numpy as np
import pytest
import torch

import select_cases as sc
from msretr._abi import MsrError
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from oracle import dense_ref

pytestmark = pytest.mark.gpu


def _tiny_index(n_docs=4):
    return CorpusIndex(doc_ids=np.arange(n_docs, dtype=np.int64), doc_len=np.ones(n_docs, np.int32),
                       term_off=np.array([0, 1], np.int64), post_doc=np.zeros(1, np.int32), post_tf=np.ones(1, np.int32),
                       idf=np.ones(1, np.float32), avgdl=1.0, total_docs=n_docs)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = DeviceEngine(_tiny_index(), max_queries=sc.MAX_QUERIES, max_k=1024)
    yield e
    e.close()


def _dev(a):
    if a is None:
        return None
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _upload(case):
    return dict(scores=_dev(case.scores), n=case.n, idx=_dev(case.idx), counts=_dev(case.counts), seg_stride=case.seg_stride,
                win_base=_dev(case.win_base), set_bits=_dev(case.set_bits), q_set=_dev(case.q_set))


def _call(eng, case, dev, **kw):
    doc, score, n, state = eng.debug_select(dev["scores"], case.k, n=dev["n"], idx=dev["idx"], counts=dev["counts"],
                                            seg_stride=dev["seg_stride"], win_base=dev["win_base"], set_bits=dev["set_bits"],
                                            q_set=dev["q_set"], **kw)
    return doc.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy(), state


def _check_rows(case, got, queries=None):
    doc, score, n, _ = got
    neg_inf = np.array(-np.inf, score.dtype)
    for q in (range(case.nq) if queries is None else queries):
        e_doc, e_score = case.expected(q)
        m = len(e_doc)
        assert n[q] == m, (case.name, q, int(n[q]), m)
        if doc[q, :m].tolist() != e_doc.tolist():
            r = int(np.nonzero(doc[q, :m] != e_doc)[0][0])
            pytest.fail(f"{case.name} query {q}: rank {r} holds document {int(doc[q, r])} score {score[q, r]!r}, expected "
                        f"document {int(e_doc[r])} score {e_score[r]!r}")
        assert sc.same_scores(score[q, :m], e_score), (case.name, q)
        assert (doc[q, m:] == -1).all() and (score[q, m:].view(np.uint8) == np.broadcast_to(neg_inf, score[q, m:].shape)
                                             .copy().view(np.uint8)).all(), (case.name, q, "padding")


def _check_state(case, state):
    """The exported SelState of every query == the model's, and the branches the case names were taken."""
    reached = set()
    for q in range(case.nq):
        _, _, m_state, tags = sc.model(case, q)
        g = tuple(int(state[q][f]) for f in sc.STATE_FIELDS)
        assert g == m_state, f"{case.name} query {q}: state {dict(zip(sc.STATE_FIELDS, g))}, the model says " \
                             f"{dict(zip(sc.STATE_FIELDS, m_state))} (branches {sorted(tags)})"
        reached |= tags
    assert case.tags <= reached, (case.name, sorted(case.tags - reached))


_SMALL = {}


def _small(eng):
    if not _SMALL:
        c = sc.build(sc.SMALL_AFTER)
        _SMALL["case"], _SMALL["dev"] = c, _upload(c)
        _SMALL["first"] = _call(eng, c, _SMALL["dev"])
        _check_rows(c, _SMALL["first"])
    return _SMALL


@pytest.mark.parametrize("name", [n for n, _ in sc.CASES])
def test_select_case_equals_reference_and_takes_its_branch(eng, name):
    case = sc.build(name)
    dev = _upload(case)
    first = _call(eng, case, dev)
    second = _call(eng, case, dev)                         # straight after: hist and cand_n must have been left all zero
    _check_rows(case, first)
    _check_state(case, first[3])
    for a, b in zip(first[:3], second[:3]):
        assert a.tobytes() == b.tobytes(), f"{name}: the second call differs from the first"
    assert first[3].tobytes() == second[3].tobytes()
    if case.big_tie:
        s = _small(eng)
        again = _call(eng, s["case"], s["dev"])
        for a, b in zip(s["first"][:3], again[:3]):
            assert a.tobytes() == b.tobytes(), f"the small case differs after {name}"


def test_gate_word_zero_leaves_outputs_alone(eng):
    case = sc.build("group_float32_5000_k10")
    dev = _upload(case)
    out = (torch.full((case.nq, case.k), 12345, dtype=torch.int32, device="cuda"),
           torch.full((case.nq, case.k), 777.0, dtype=torch.float32, device="cuda"),
           torch.full((case.nq,), -99, dtype=torch.int32, device="cuda"))
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    _call(eng, case, dev, gate=gate, out=out)
    assert (out[0] == 12345).all() and (out[1] == 777.0).all() and (out[2] == -99).all()
    _check_rows(case, _call(eng, case, dev))                # the next ungated call
    gate.fill_(1)
    _check_rows(case, _call(eng, case, dev, gate=gate, out=out))


def test_gate_per_64_queries(eng):
    """nq = 130: slices 0 (queries 0-63) and 2 (128, 129) on, slice 1 (64-127) off."""
    x = sc.random_rows(np.float32, 130, 9000, 71)
    x[5] = 0.5                                              # a tie group above the cap in an ON slice
    x[70] = 0.25                                            # ... and in the OFF slice
    case = sc.Case("gate_per64", x, 100, set())
    dev = _upload(case)
    out = (torch.full((130, 100), 12345, dtype=torch.int32, device="cuda"),
           torch.full((130, 100), 777.0, dtype=torch.float32, device="cuda"),
           torch.full((130,), -99, dtype=torch.int32, device="cuda"))
    gate = torch.tensor([1, 0, 5], dtype=torch.int32, device="cuda")
    got = _call(eng, case, dev, gate=gate, gate_per64=True, out=out)
    on = list(range(64)) + [128, 129]
    _check_rows(case, got, on)
    assert (got[0][64:128] == 12345).all() and (got[1][64:128] == 777.0).all() and (got[2][64:128] == -99).all()
    _check_rows(case, _call(eng, case, dev))                # all queries, ungated, straight after


def test_debug_select_refusals(eng):
    x = torch.zeros((2, 100), dtype=torch.float32, device="cuda")
    x64 = x.double()
    idx = torch.zeros((2, 100), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    out = (torch.full((2, 10), 7, dtype=torch.int32, device="cuda"), torch.full((2, 10), 7.0, device="cuda"),
           torch.full((2,), 7, dtype=torch.int32, device="cuda"))
    for kw in (dict(k=0), dict(k=1025), dict(k=10, n=101), dict(k=10, n=-1)):
        with pytest.raises(MsrError) as ei:
            eng.debug_select(x, kw.pop("k"), out=out, **kw)
        assert ei.value.code == -1
    with pytest.raises(MsrError):
        eng.debug_select(x64, 10, idx=idx, counts=cnt, seg_stride=26)            # 4 x 26 > stride
    with pytest.raises(MsrError):
        eng.debug_select(x64, 10, idx=idx, counts=cnt[:, :0], seg_stride=1)       # n_seg = 0
    with pytest.raises(MsrError):
        eng.debug_select(torch.zeros((sc.MAX_QUERIES + 1, 8), device="cuda"), 1)
    assert (out[0] == 7).all() and (out[1] == 7.0).all() and (out[2] == 7).all()


def test_bm25_topk_equals_select_on_its_own_candidate_row():
    """msr_bm25_topk == msr_debug_select over the row rebuilt from msr_bm25_score_docs (the same scores bit for bit): the
    touched documents with score >= 0 as one list segment."""
    from msretr.synthetic import synthetic_corpus, synthetic_queries
    ix = synthetic_corpus(6000, n_chunks=6000, n_terms=3000, seed=13)
    terms, _ = synthetic_queries(ix, 3, seed=14)
    e = DeviceEngine(ix, max_queries=8, max_k=1000)
    N = ix.n_docs
    for k in (10, 1000):
        doc, score, n = [t.cpu().numpy() for t in e.bm25_topk(terms, k=k)]
        all_docs = torch.arange(N, dtype=torch.int32, device="cuda").repeat(len(terms), 1)
        s, touched = e.bm25_score_docs(terms, all_docs)
        s, touched = s.cpu().numpy(), touched.cpu().numpy()
        sc_rows = np.full((len(terms), N), 1e300)
        ix_rows = np.zeros((len(terms), N), np.int32)
        counts = np.zeros((len(terms), 1), np.int32)
        for q in range(len(terms)):
            keep = np.nonzero((touched[q] != 0) & (s[q] >= 0.0))[0][::-1]           # (any order)
            sc_rows[q, :len(keep)], ix_rows[q, :len(keep)], counts[q, 0] = s[q, keep], keep, len(keep)
        d2, s2, n2, _ = e.debug_select(_dev(sc_rows), k, idx=_dev(ix_rows), counts=_dev(counts), seg_stride=N)
        assert n.tobytes() == n2.cpu().numpy().tobytes() and doc.tobytes() == d2.cpu().numpy().tobytes()
        assert score.tobytes() == s2.cpu().numpy().tobytes()
        assert (n > 0).all()
    e.close()


# ------------------------------------------------------------------------------------------------------------------ merges
class _Gathered:
    """The receive buffer of an all-gather, shaped like distributed._Exchange: `world` records of [doc | score | n | pay],
    every segment 8-byte aligned, `lead` unrelated bytes in front of each record's first segment."""

    def __init__(self, docs, scores, ns, pays, lead=0):
        self.world, self.Q, k = docs.shape[:3]
        self.off, o = {}, lead
        for name, a in (("doc", docs), ("score", scores), ("n", ns), ("pay", pays)):
            self.off[name] = (o, a.dtype, a.shape[1:])
            o += (a[0].nbytes + 7) // 8 * 8
        self.record = o
        host = np.full((self.world, o), 0xA5, np.uint8)
        for name, a in (("doc", docs), ("score", scores), ("n", ns), ("pay", pays)):
            b = self.off[name][0]
            for g in range(self.world):
                host[g, b:b + a[g].nbytes] = np.ascontiguousarray(a[g]).view(np.uint8).reshape(-1)
        self.recv = torch.from_numpy(host.reshape(-1)).cuda()

    def part(self, g, name):
        o, dt, shape = self.off[name]
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        t = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dt)]
        return self.recv[g * self.record + o: g * self.record + o + nb].view(t).view(*shape)


def _pay_of(doc):
    return ((doc.astype(np.int64) * 7 + 3) & 0x7FFFFFFF).astype(np.int32)


def _lists(rng, G, Q, k, dt, shape):
    """Sorted per-shard lists (documents unique across shards).  shape: 'alike' (the counting merge takes these), 'skewed'
    (one list holds all of the best: quota > SPEC, the counting merge declines), 'ragged' (random lengths, many ties)."""
    docs = np.full((G, Q, k), -1, np.int32); sco = np.full((G, Q, k), -np.inf, dt); ns = np.zeros((G, Q), np.int32)
    for g in range(G):
        for q in range(Q):
            m = int(rng.integers(0, k + 1)) if shape == "ragged" else k
            if shape == "ragged":
                s = rng.integers(0, 50, size=m).astype(dt) / dt(7)
            else:
                s = (rng.standard_normal(m) + (8.0 if shape == "skewed" and g == G - 1 else 0.0)).astype(dt)
            d = rng.choice(np.arange(g * 100000, (g + 1) * 100000), size=m, replace=False).astype(np.int32)
            o = np.lexsort((d, -s.astype(np.float64)))
            docs[g, q, :m], sco[g, q, :m], ns[g, q] = d[o], s[o], m
    return docs, sco, ns


def _expected_merge(docs, sco, ns, k, q):
    parts = []
    for g in range(docs.shape[0]):
        c = min(max(int(ns[g, q]), 0), k)
        d, s = docs[g, q, :c].astype(np.int64), sco[g, q, :c]
        ok = ~np.isnan(s) & (s != -np.inf)
        parts.append((d[ok], s[ok]))
    return dense_ref.merge_topk(parts, k)


def _check_merge(eng, docs, sco, ns, k, payload, lead, what):
    G, Q = docs.shape[:2]
    ex = _Gathered(docs, sco, ns, _pay_of(docs), lead)
    od, os_, on, op = eng.merge_gathered(ex, "doc", "score", "n", "pay" if payload else None, k)
    od, os_, on = od.cpu().numpy(), os_.cpu().numpy(), on.cpu().numpy()
    assert (op is not None) == payload
    for q in range(Q):
        e_doc, e_score = _expected_merge(docs, sco, ns, k, q)
        m = len(e_doc)
        assert on[q] == m, (what, q, int(on[q]), m)
        assert od[q, :m].tolist() == e_doc.tolist(), (what, q)
        assert sc.same_scores(os_[q, :m], e_score.astype(sco.dtype)), (what, q)
        assert (od[q, m:] == -1).all() and np.isneginf(os_[q, m:]).all(), (what, q, "padding")
        if payload:
            p = op.cpu().numpy()
            assert p[q, :m].tolist() == _pay_of(e_doc).tolist() and (p[q, m:] == -1).all(), (what, q, "payload")


def _served(G, k):
    lists, entries = 1, 64
    while lists < G:
        lists <<= 1
    while entries < k:
        entries <<= 1
    return lists * entries <= 8192


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("payload", [False, True])
def test_merge_gathered_in_place(eng, dt, payload):
    rng = np.random.default_rng(3)
    for G in (1, 2, 3, 8, 64):
        for k in (1, 37, 64, 65, 1000, 1024):
            if G * k > 8192 or not _served(G, k):
                continue                                    # (refusals: test_merge_limit_is_refused_before_any_launch)
            for shape in ("alike", "skewed", "ragged"):
                docs, sco, ns = _lists(rng, G, 2, k, dt, shape)
                _check_merge(eng, docs, sco, ns, k, payload, 24 if shape != "ragged" else 0, (G, k, shape))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_merge_invalid_scores_and_clamped_counts(eng, dt):
    rng = np.random.default_rng(4)
    G, Q, k = 8, 6, 100
    docs, sco, ns = _lists(rng, G, Q, k, dt, "alike")
    sco[2, 0, 3] = np.nan                                   # inside the counted prefix: the query goes to the merge tree
    sco[5, 0, k - 2:] = -np.inf                             # (a sorted list can hold -inf at its end only)
    sco[1, 1, k - 1] = -np.inf
    sco[6, 1, k - 1] = np.nan
    ns[:, 2] = [-3, 0, k, k + 5, 1, -1, k + 1000, 7]        # counts outside [0, k] clamp
    ns[:, 3] = 0                                            # all lists empty
    ns[:, 4] = -3
    for g, z in ((3, -0.0), (4, 0.0)):                      # two lists of zeros of either sign: one key, documents decide
        sco[g, 5, :] = z
        docs[g, 5, :] = np.sort(docs[g, 5, :])
    for payload in (False, True):
        _check_merge(eng, docs, sco, ns, k, payload, 8, ("invalid", dt.__name__, payload))


def test_merge_short_lists_with_an_invalid_entry(eng):
    """Fewer than k entries in all and a NaN among them: out_n counts the entries that remain."""
    rng = np.random.default_rng(8)
    for dt in (np.float32, np.float64):
        docs, sco, ns = _lists(rng, 3, 2, 100, dt, "alike")
        ns[:] = 10
        sco[1, 0, 4] = np.nan
        sco[2, 1, 9] = -np.inf
        _check_merge(eng, docs, sco, ns, 100, True, 0, ("short", dt.__name__))


def test_merge_duplicate_documents_keep_both_entries(eng):
    """What msretr.h defines for the same document in two lists: no de-duplication, equal keys adjacent."""
    k = 10
    docs = np.tile(np.arange(100, 100 + k, dtype=np.int32)[None, None, :], (2, 1, 1))
    sco = np.tile(np.arange(k, 0, -1, dtype=np.float32)[None, None, :], (2, 1, 1))
    ns = np.full((2, 1), k, np.int32)
    t = lambda a: torch.as_tensor(a).cuda()
    od, os_, on = [x.cpu().numpy() for x in eng.merge_topk(t(docs), t(sco), t(ns), k)]
    assert on[0] == k and od[0].tolist() == np.repeat(np.arange(100, 105), 2).tolist()
    assert os_[0].tolist() == np.repeat(np.arange(k, k - 5, -1), 2).astype(np.float32).tolist()


def test_merge_limit_is_refused_before_any_launch(eng):
    """Every (n_parts, k) is either served exactly or refused with MSR_ERR_INVALID and the limit in the message, outputs
    untouched: pow2ceil(n_parts) * max(64, pow2ceil(k)) <= 8192.  (17, 480) = 32 x 512 and its neighbours pin it."""
    rng = np.random.default_rng(6)
    pinned = {(17, 480): False, (16, 480): True, (17, 256): True, (17, 257): False, (16, 512): True, (17, 481): False,
              (32, 256): True, (33, 128): True, (33, 129): False, (12, 600): False, (8, 1024): True, (9, 600): False}
    for (G, k), ok in pinned.items():
        assert _served(G, k) == ok
    for G in (1, 2, 3, 5, 8, 9, 12, 16, 17, 32, 33, 64):
        for k in (1, 37, 64, 65, 128, 129, 256, 257, 480, 481, 512, 513, 600, 1000, 1024):
            docs, sco, ns = _lists(rng, G, 1, k, np.float32, "alike")
            if _served(G, k):
                _check_merge(eng, docs, sco, ns, k, True, 0, (G, k))
                continue
            t = lambda a: torch.as_tensor(a).cuda()
            out = [torch.full((1, k), 7, dtype=torch.int32, device="cuda"), torch.full((1, k), 7.0, device="cuda"),
                   torch.full((1,), 7, dtype=torch.int32, device="cuda")]
            import ctypes as C
            p = lambda x: C.c_void_p(x.data_ptr())
            d_, s_, n_ = t(docs), t(sco), t(ns)
            rc = eng.lib.msr_merge_topk(eng.handle, p(d_), p(s_), p(n_), G, 1, k, 32, p(out[0]), p(out[1]), p(out[2]), eng._stream())
            msg = eng.lib.msr_last_error(eng.handle).decode()
            assert rc == -1 and "8192" in msg and "powers of two" in msg, (G, k, rc, msg)
            torch.cuda.synchronize()
            assert (out[0] == 7).all() and (out[1] == 7.0).all() and (out[2] == 7).all(), (G, k)
