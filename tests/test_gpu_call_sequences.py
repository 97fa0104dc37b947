"""No engine call leaves state behind for the next one (tests/call_sequence_cases.py: the probes, the dirtiers, the bundles).

A  each probe, made as the first call after a fresh bind, gives its CLEAN bytes; they are checked against the CPU oracles
   the suite already uses for that call (BM25 and the select bit for bit, the dense calls at the project's 1e-5 with ties as
   test_gpu_parity.py handles them, the rerank chain at RERANK_BAR), so they are not merely self-consistent.
B  after every dirtier its path predicate holds, every count of DeviceEngine.scratch_dirty() is 0 (or -1: not allocated)
   and split_pending is what the dirtier says.
C  the full matrix on the long-lived engines: every dirtier followed by every probe, whose outputs must equal the clean bytes
   byte for byte, padding included; then three seeded sequences of 200 calls drawn from both lists, scratch_dirty() checked
   after every step and every probe compared.  Every probe of the catalogue is byte-deterministic: the streaming passes and
   the bf16 GEMM bucket their entries with atomics, but every list they return is sorted by (exact f32 score, document) at
   the end, and the BM25 stage and the select use no floating-point atomics at all -- so no probe is compared at a bar.
D  msr_debug_count_nonzero on torch buffers: the negative control of B -- the counter does see dirt.
"""
import time

import numpy as np
import pytest
import torch

import call_sequence_cases as cs
import select_cases as S
from msretr import _abi
from msretr.engine import count_nonzero_words
from oracle import bm25_ref, dense_ref
from within_ref import restrict_list

pytestmark = pytest.mark.gpu

RERANK_BAR = 5e-6          # tests/test_gpu_hybrid.py, test_gpu_parity.py
DENSE_TOL = 1e-5           # the project's stated dense tolerance
TIE = 4e-6                 # test_batched_gemm_path_equals_exact_scan: neighbours this close may swap
COUNTED = [n for n in _abi.MSR_DIRTY_NAMES if n != "split_pending"]


# ------------------------------------------------------------------------------------------------------------ the bundles
class _Bundles:
    def __init__(self):
        self.b = {}

    def get(self, name):
        """The bundle, made on first use, with the clean bytes of its probes: each probe as the FIRST call after a fresh bind."""
        if name not in self.b:
            t0 = time.time()
            b = cs.Bundle(name)
            for p in cs.entries_for(name, "probe"):
                b.fresh()
                b.clean[p.name], _ = p.run(b)
                _assert_clean_scratch(b, p.name, "as the first call after a bind", pending=0)
            b.fresh()
            print(f"bundle {name}: engine, inputs and {len(b.clean)} clean probes in {time.time() - t0:.1f} s")
            self.b[name] = b
        return self.b[name]

    def close(self):
        for b in self.b.values():
            b.close()


@pytest.fixture(scope="module")
def bundles():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    bs = _Bundles()
    yield bs
    bs.close()


def _assert_clean_scratch(b, name, when, pending):
    d = b.eng.scratch_dirty()
    for buf in COUNTED:
        assert d[buf] in (0, -1), f"bundle {b.name}: {d[buf]} non-zero words in {buf} after {name} ({when}); all: {d}"
    assert d["split_pending"] == pending, f"bundle {b.name}: split_pending = {d['split_pending']} after {name} ({when}), " \
                                          f"expected {pending}"


def _diff(got, clean, prefix=""):
    """-> the names of the outputs whose bytes differ (nested dicts walked)."""
    bad = []
    for k in clean:
        if isinstance(clean[k], dict):
            bad += _diff(got[k], clean[k], prefix + k + ".")
        elif got[k].shape != clean[k].shape or got[k].dtype != clean[k].dtype or got[k].tobytes() != clean[k].tobytes():
            bad.append(prefix + k)
    return bad


def _where(got, clean, key):
    a, c = got[key], clean[key]
    if a.shape != c.shape:
        return f"shape {a.shape} != {c.shape}"
    v = a.reshape(len(a), -1).view(np.uint8) != c.reshape(len(c), -1).view(np.uint8)
    rows = np.nonzero(v.any(axis=1))[0]
    r = int(rows[0])
    return f"{len(rows)} of {len(a)} rows differ; first: row {r}: {a[r].reshape(-1)[:8].tolist()} != clean {c[r].reshape(-1)[:8].tolist()}"


# ------------------------------------------------------------------------------------------------------------ A: oracles
def _check_select(b, name, out):
    case = cs.select_case(cs.SELECT_PROBES[name])
    neg_inf = np.array(-np.inf, out["score"].dtype)
    for q in range(case.nq):
        e_doc, e_score = case.expected(q)
        m = len(e_doc)
        assert out["n"][q] == m and out["doc"][q, :m].tolist() == e_doc.tolist(), (name, q)
        assert S.same_scores(out["score"][q, :m], e_score), (name, q)
        assert (out["doc"][q, m:] == -1).all() and (out["score"][q, m:] == neg_inf).all(), (name, q, "padding")


def _check_merge(b, name, out):
    docs, sco, ns = cs.merge_lists_input()
    for q in range(docs.shape[1]):
        e_doc, e_score = dense_ref.merge_topk([(docs[g, q].astype(np.int64), sco[g, q]) for g in range(docs.shape[0])], 37)
        assert out["n"][q] == 37 and out["doc"][q].tolist() == e_doc.tolist() and S.same_scores(out["score"][q], e_score), q


def _bm25_rows(out, exp, what):
    e_doc, e_score, e_n = exp
    assert out["n"].tolist() == e_n.tolist(), what
    assert out["doc"].tobytes() == e_doc.tobytes(), what
    assert out["score"].view(np.int64).tobytes() == e_score.view(np.int64).tobytes(), what       # (padding included)


def _check_bm25(b, name, out):
    i = b.inp
    _bm25_rows(out, cs.sc.expected_rows([bm25_ref.topk(i.z, i.queries[j], cs.K_BM25) for j in i.mixed16], cs.K_BM25), name)
    assert out["n"].max() == cs.K_BM25


def _check_bm25_within(b, name, out):
    i = b.inp
    rows = []
    for j, s in zip(i.mixed16, i.within_names(16)):
        fd, fs = bm25_ref.topk(i.z, i.queries[j], i.n_docs)
        rows.append((fd[:cs.K_BM25], fs[:cs.K_BM25]) if i.masks[s] is None else restrict_list(fd, fs, len(fd), i.masks[s], cs.K_BM25))
    _bm25_rows(out, cs.sc.expected_rows(rows, cs.K_BM25), name)
    assert all(len(r[0]) == 0 for r, s in zip(rows, i.within_names(16)) if s == "empty")


_BEST = {}


def _best(b, idx):
    """dense_ref.doc_scores of distinct query idx of the bundle: (best float32 [N], arg-max row [N]), evaluated once."""
    key = (b.name, idx)
    if key not in _BEST:
        _BEST[key] = dense_ref.doc_scores(b.inp.emb, b.inp.doc_off, b.inp.distinct[idx])
    return _BEST[key]


def _ranked(best, k, mask=None):
    cand = np.nonzero(np.isfinite(best) & (True if mask is None else mask))[0]
    sel = cand[np.argsort(-best[cand], kind="stable")[:k]]
    return sel, best[sel]


def _dense_row(b, what, doc, score, chunk, n, oi, os_, arg, best, rows=None):
    """One row against the oracle's list at the project's bar: the count, every score within 1e-5, the documents equal
    except where the oracle's neighbouring scores lie within 4e-6 of each other -- and there the document that stands in must
    be one of the tie group: its own oracle score (best[d]; -inf outside the query's set) within 4e-6 of the oracle's score at
    that rank, and no document twice; the arg-max row inside its document.  rows (list): receives (agreeing, compared)
    arg-max rows, summed over the probe by the caller (test_batched_gemm_path_equals_exact_scan's 99.9 %)."""
    assert n == len(oi), (what, int(n), len(oi))
    assert np.abs(score[:n].astype(np.float64) - os_).max(initial=0.0) <= DENSE_TOL, what
    near = (np.abs(np.r_[np.diff(os_), 1.0]) <= TIE) | (np.abs(np.r_[1.0, np.diff(os_)]) <= TIE)
    assert ((doc[:n] == oi) | near).all(), (what, doc[:n].tolist(), oi.tolist())
    moved = doc[:n] != oi
    assert (np.abs(best[doc[:n][moved].astype(np.int64)].astype(np.float64) - os_[moved]) <= TIE).all(), (what, "not of the tie group")
    assert len(set(doc[:n].tolist())) == n, (what, "a document twice")
    assert (doc[n:] == -1).all() and np.isneginf(score[n:]).all(), (what, "padding")
    if chunk is not None:
        off = b.inp.doc_off
        d = doc[:n].astype(np.int64)
        assert ((chunk[:n] >= off[d]) & (chunk[:n] < off[d + 1])).all(), (what, "arg-max row outside its document")
        if rows is not None:
            rows.append((int((chunk[:n] == arg[d]).sum()), int(n)))
        assert (chunk[n:] == -1).all()


def _check_dense(Q, shift=0, within=False):
    def check(b, name, out):
        idx, _ = b.inp.rows(Q, shift)
        sets = b.inp.within_names(Q) if within else [None] * Q
        rows = []
        for r, (i, s) in enumerate(zip(idx, sets)):
            best, arg = _best(b, i)
            mask = None if s is None or b.inp.masks[s] is None else b.inp.masks[s]
            oi, os_ = _ranked(best, cs.K_DENSE, mask)
            _dense_row(b, (name, r), out["doc"][r], out["score"][r], out.get("chunk", [None] * Q)[r], out["n"][r], oi, os_, arg,
                       best if mask is None else np.where(mask, best, -np.inf), rows)
        agree, compared = sum(a for a, _ in rows), sum(c for _, c in rows)
        # the arg-max row of every returned document is the oracle's first arg-max row of THAT document, 99.9 % of the time
        # (two rows of one document within rounding of each other may swap)
        assert agree >= 0.999 * compared, (name, "arg-max rows", agree, compared)
        if within:
            assert [int(out["n"][r]) for r, s in enumerate(sets) if s == "empty"] == [0] * sets.count("empty")
    return check


def _check_split(b, name, out):
    _check_dense(100)(b, name, {k: out[k] for k in ("doc", "score", "chunk", "n")})
    idx, _ = b.inp.rows(100)
    for r, i in enumerate(idx):                                # part: a cosine that k documents of this shard reach exactly
        _, os_ = _ranked(_best(b, i)[0], cs.K_DENSE)
        assert out["part"][r] <= os_[-1] + DENSE_TOL, (name, r)


def _check_grouped(b, name, out):
    idx, _ = b.inp.rows(20, 2)
    goff = cs.GROUP_OFF
    for g in range(len(goff) - 1):
        r0, r1 = int(goff[g]), int(goff[g + 1])
        if r1 == r0:
            assert out["n"][g] == 0
            continue
        Sg = np.stack([_best(b, idx[r])[0] for r in range(r0, r1)])
        best = Sg.max(axis=0)
        best[cs.GROUP_EXCL[g]] = -np.inf
        oi, os_ = _ranked(best, cs.K_DENSE)
        _dense_row(b, (name, g), out["doc"][g], out["score"][g], None, out["n"][g], oi, os_, None, best)
        for j in range(int(out["n"][g])):
            r, d = int(out["src"][g, j]), int(out["doc"][g, j])
            assert r0 <= r < r1 and abs(float(Sg[r - r0, d]) - float(best[d])) <= 2 * DENSE_TOL, (name, g, j)
            assert d not in cs.GROUP_EXCL[g]


def _check_union(b, name, out):
    """The CPU chain's candidate lists (hybrid_ref.candidates: the planted dense winners are unambiguous): exact."""
    import hybrid_ref as H
    i = b.inp
    cd, cs_, csrc, cn = i.candidates()
    assert out["n"].tolist() == cn.tolist() and out["doc"].tobytes() == cd.tobytes() and out["src"].tobytes() == csrc.tobytes()
    assert out["score"].view(np.int64).tobytes() == cs_.view(np.int64).tobytes()
    for q in range(len(i.terms)):
        dd, _, _ = dense_ref.quick_search(i.emb, i.doc_off, i.qv[q], i.dense_k)
        ws, wt = H.point_scores(i.z, i.terms[q], dd)
        assert out["point_score"][q].tolist() == ws.tolist() and out["point_touched"][q].tolist() == wt.astype(np.int32).tolist(), q


_CHAIN = {}


def _cpu_chain(b):
    """The rerank chain on the CPU (hybrid_ref.fused = oracle.rerank_ref), then the engine's diversify over it, as
    test_hybrid_step_against_the_cpu_chain builds its expectation -> (fused host arrays, final host arrays)."""
    if "v" not in _CHAIN:
        import hybrid_ref as H
        from oracle_engine import OracleEngine
        i, e, cfg = b.inp, b.eng, b.retriever.reranker.cfg
        cd, cs_, _, cn = i.candidates()
        fused = H.fused(OracleEngine(i.ix), cd, cs_, cn, i.qv, smoothing=cfg["smoothing"])
        dts = (torch.int32, torch.float64, torch.float64, torch.int32, torch.int32)
        dev = tuple(x.to(device=e.device, dtype=dt).contiguous() for x, dt in zip(fused, dts))
        b.retriever._ensure_response_tables()
        fin = e.diversify(dev, top_k=int(cfg["top_k"]), diversification=bool(cfg.get("diversification", False)))
        _CHAIN["v"] = ([x.cpu().numpy() for x in dev], [x.cpu().numpy() for x in fin])
    return _CHAIN["v"]


def _lists_at_bar(what, doc, score, n, wd, ws, wn, exact_order=True):
    """The counts; every document's score within RERANK_BAR of the CPU chain's; the order equal -- exact_order=False (lists of
    a thousand fused candidates, where scores do fall within the bar of each other): equal outside the tie bar, that is a
    document may stand elsewhere only among neighbours whose CPU scores lie within 2 RERANK_BAR of its own."""
    assert n.tolist() == wn.tolist(), what
    worst = 0.0
    for q in range(len(n)):
        k = int(n[q])
        if exact_order:
            assert doc[q, :k].tolist() == wd[q, :k].tolist(), (what, q)
            worst = max(worst, float(np.abs(score[q, :k] - ws[q, :k]).max()) if k else 0.0)
            continue
        want = dict(zip(wd[q, :k].tolist(), ws[q, :k].tolist()))
        assert sorted(want) == sorted(doc[q, :k].tolist()), (what, q)
        got_cpu = np.array([want[d] for d in doc[q, :k].tolist()])
        worst = max(worst, float(np.abs(score[q, :k] - got_cpu).max()) if k else 0.0)
        moved = doc[q, :k] != wd[q, :k]
        assert (np.abs(got_cpu[moved] - ws[q, :k][moved]) <= 2 * RERANK_BAR).all(), (what, q, "order outside the tie bar")
    assert worst <= RERANK_BAR, (what, worst)


def _check_rerank(b, name, out):
    fused, fin = _cpu_chain(b)
    _lists_at_bar(name + " fused", out["f_doc"], out["f_score"], out["f_n"], fused[0], fused[1], fused[4], exact_order=False)
    _lists_at_bar(name + " final", out["doc"], out["score"], out["n"], fin[0], fin[1], fin[4])


def _check_final(b, name, out):
    _, fin = _cpu_chain(b)
    _lists_at_bar(name, out["doc"], out["score"], out["n"], fin[0], fin[1], fin[4])
    chain = b.clean["rerank_chain"]                            # and the step IS its parts: the same bytes as the rerank probe
    for q in range(len(out["n"])):
        k = int(out["n"][q])
        assert out["doc"][q, :k].tobytes() == chain["doc"][q, :k].tobytes() and \
            out["score"][q, :k].tobytes() == chain["score"][q, :k].tobytes() and \
            out["chunk"][q, :k].tobytes() == chain["chunk"][q, :k].tobytes(), q
    assert out["n"].max() > 0 and out["n"][3] > 0 and set(np.unique(out["src"])) <= {0, 1, 2, 3}


ORACLES = {
    "select_f32": _check_select, "select_f64_list": _check_select, "merge_topk": _check_merge,
    "bm25_topk_16": _check_bm25, "bm25_topk_within": _check_bm25_within,
    "dense_topk_8": _check_dense(8), "dense_topk_100": _check_dense(100), "dense_topk_200": _check_dense(200),
    "dense_topk_within": _check_dense(16, 1, within=True),
    "dense_topk_batched_100": _check_dense(100), "dense_topk_batched_200": _check_dense(200),
    "dense_topk_grouped": _check_grouped, "dense_begin_end": _check_split,
    "score_docs_union": _check_union, "rerank_chain": _check_rerank, "final_lists_hybrid": _check_final,
}
EXPECTED_PATH = {"dense_topk_8": 64, "dense_topk_100": 128, "dense_topk_200": 256, "dense_begin_end": 128}


@pytest.mark.parametrize("bundle", cs.ALL)
def test_clean_answers_match_the_oracles(bundles, bundle):
    assert set(ORACLES) == {p.name for p in cs.PROBES}, "a probe without an oracle"
    b = bundles.get(bundle)
    for p in cs.entries_for(bundle, "probe"):
        ORACLES[p.name](b, p.name, b.clean[p.name])
    # the probes took the paths they are named for (read once more, on the live engine)
    for p in cs.entries_for(bundle, "probe"):
        if p.name in EXPECTED_PATH:
            _, rep = p.run(b)
            assert rep["dense_path"] == EXPECTED_PATH[p.name], (p.name, rep)
        if p.name.startswith("dense_topk_batched"):
            _, rep = p.run(b)
            assert rep["batch_width"] == 128 and rep["gemm_ok"], rep
    if bundle in cs.DENSE:
        assert b.eng.scan_width() == 256 and b.eng.scan_arith() == "f16x2"


# ------------------------------------------------------------------------------------------------------------ B
PAIRS = [(bn, g) for bn in cs.ALL for g in cs.GROUPS if cs.entries_for(bn, "dirtier", g)]


@pytest.mark.parametrize("bundle,group", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_dirtier_keeps_the_invariants(bundles, bundle, group):
    b = bundles.get(bundle)
    for d in cs.entries_for(bundle, "dirtier", group):
        out, rep = d.run(b)
        _assert_clean_scratch(b, d.name, "dirtier", d.pending)
        try:
            d.check(b, out, rep)
        except AssertionError as e:
            raise AssertionError(f"bundle {bundle}: the path predicate of dirtier {d.name} does not hold: {e}") from e
        out2, _ = d.run(b)                                     # and straight after itself: the same bytes
        assert not _diff(out2, out), f"bundle {bundle}: dirtier {d.name} differs when repeated: {_diff(out2, out)}"
        _assert_clean_scratch(b, d.name, "dirtier, repeated", d.pending)


# ------------------------------------------------------------------------------------------------------------ C
def _run_probe(b, p, context):
    got, _ = p.run(b)
    bad = _diff(got, b.clean[p.name])
    if bad:
        return f"bundle {b.name}: probe {p.name} {context}: outputs {bad} differ from the clean bytes ({_where(got, b.clean[p.name], bad[0]) if '.' not in bad[0] else ''})"
    return None


@pytest.mark.parametrize("bundle,group", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_probe_after_every_dirtier(bundles, bundle, group):
    b = bundles.get(bundle)
    probes = cs.entries_for(bundle, "probe")
    for d in cs.entries_for(bundle, "dirtier", group):
        for p in probes:
            d.run(b)
            _assert_clean_scratch(b, d.name, "dirtier, before probe " + p.name, d.pending)
            msg = _run_probe(b, p, f"after dirtier {d.name}")
            assert msg is None, msg
            _assert_clean_scratch(b, p.name, "probe after dirtier " + d.name, 0)


def _replay(b, names):
    """The steps from a fresh bind -> the failure message of the LAST step (None: it passes)."""
    b.fresh()
    msg = None
    for nm in names:
        e = cs.by_name(nm)
        msg = None
        if e.kind == "probe":
            msg = _run_probe(b, e, "in a replay")
        else:
            e.run(b)
        d = b.eng.scratch_dirty()
        if msg is None and any(d[x] not in (0, -1) for x in COUNTED):
            msg = f"scratch dirty after {nm}: {d}"
    return msg


def _shortest_suffix(b, steps, t):
    for L in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, t + 1):
        L = min(L, t + 1)
        if _replay(b, steps[t + 1 - L:t + 1]) is not None:
            return steps[t + 1 - L:t + 1]
        if L == t + 1:
            break
    return None


SEQS = [(bn, s) for bn in cs.ALL for s in cs.SEQUENCE_SEEDS]


@pytest.mark.parametrize("bundle,seed", SEQS, ids=["%s-%d" % p for p in SEQS])
def test_seeded_sequences(bundles, bundle, seed):
    """200 calls drawn from the probes and the dirtiers of the bundle: scratch_dirty() after every step, every probe compared
    with its clean bytes.  A failure names the seed, the step, the last dirtier before it and the shortest suffix of the
    sequence that reproduces it from a fresh bind."""
    b = bundles.get(bundle)
    steps = cs.seeded_sequence(seed, bundle)
    last_dirtier = None
    for t, nm in enumerate(steps):
        e = cs.by_name(nm)
        msg = None
        if e.kind == "probe":
            msg = _run_probe(b, e, f"at step {t}")
        else:
            e.run(b)
            last_dirtier = nm
        d = b.eng.scratch_dirty()
        if msg is None and (any(d[x] not in (0, -1) for x in COUNTED) or d["split_pending"] != 0):
            msg = f"bundle {bundle}: scratch_dirty() after step {t} ({nm}): {d}"
        if msg is not None:
            suffix = _shortest_suffix(b, steps, t)
            pytest.fail(f"seed {seed}, step {t} ({nm}), last dirtier before it: {last_dirtier}: {msg}\nshortest suffix that "
                        f"reproduces it from a fresh bind: {suffix if suffix is not None else 'none up to the whole prefix (order- or history-dependent)'}")


# ------------------------------------------------------------------------------------------------------------ D
def test_the_counter_counts():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda", 0)
    hist = cs.MAX_QUERIES * cs.caps()["sel_bins"]              # the extent of sel.hist on the bundles' engines
    for n in (0, 1, 255, 256, 257, hist):
        z = torch.zeros((n,), dtype=torch.int32, device=dev)
        assert count_nonzero_words(z) == 0, n
        if n == 0:
            continue
        for at in sorted({0, n - 1, min(255, n - 1), min(256, n - 1), min(256 * 1024 - 1, n - 1), min(256 * 1024, n - 1), n // 2}):
            z.zero_()
            z[at] = 7
            assert count_nonzero_words(z) == 1, (n, at)         # one word: the first, the last, both sides of a block edge
        z.zero_()
        marks = sorted({0, n - 1, n // 3, min(255, n - 1), min(256, n - 1)})
        z[marks] = -1
        assert count_nonzero_words(z) == len(marks), n
        z.fill_(3)
        assert count_nonzero_words(z) == n, n                  # every word
        assert count_nonzero_words(z, n_words=n - 1) == n - 1 and count_nonzero_words(z[1:]) == n - 1      # only the extent asked for
    f = torch.zeros((257,), dtype=torch.float32, device=dev)
    f[5] = -0.0                                                # bits 0x80000000: equal to zero as a float, dirt as a word
    f[256] = float("nan")
    assert int(f.view(torch.int32)[5]) == -2 ** 31 and count_nonzero_words(f) == 2
    d = torch.zeros((4,), dtype=torch.float64, device=dev)
    d[1] = 1.0                                                 # 0x3FF00000 00000000: one of its two words
    assert count_nonzero_words(d) == 1
    lib = _abi.load()
    out = torch.zeros((1,), dtype=torch.int64, device=dev)
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.msr_debug_count_nonzero(P(f), -1, P(out), st) == -1
    assert lib.msr_debug_count_nonzero(None, 4, P(out), st) == -1
    assert lib.msr_debug_count_nonzero(P(f), 4, None, st) == -1
    assert lib.msr_debug_count_nonzero(C.c_void_p(f.data_ptr() + 2), 4, P(out), st) == -1
    assert lib.msr_debug_count_nonzero(None, 0, P(out), st) == 0 and int(out.item()) == 0
