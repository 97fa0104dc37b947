"""The catalogue of the call-sequence tests (test_call_sequence_cases.py on the CPU, test_gpu_call_sequences.py on the GPU).

An engine carries state from one call to the next: scratch documented "zero between calls" that every kernel must put back on
every exit, one set of score rows and one select scratch shared by all the top-k entry points, a pending dense_begin.  The
symptom of a broken invariant is a wrong row in some LATER, unrelated call, so the tests here never look at one call alone:

PROBES    one ordinary call per stage.  Made first after a fresh bind they give the CLEAN bytes (checked against the CPU
          oracles by the GPU test); made after anything else they must give the same bytes.
DIRTIERS  every call that leaves by an unusual path -- an overflow, a raised or unraised gate, a query that is done early, an
          empty set, fewer queries after more, a refused call, a rebind -- each with a predicate on its own outputs or on the
          engine's reports that proves the path was taken.

Every entry is a function of a Bundle (one long-lived engine on one index plus its inputs) and returns the host arrays of its
outputs and a dict of what the engine reported.  The inputs are the suite's existing small fixtures recombined: the 61-tile
BM25 corpus of bm25_span_cases.py ("lex"), the f16 and bf16 corpora of dense_adversary.py with their 5500-document twin group
("f16", "bf16"), the raw-row cases of select_cases.py picked by their tags, and a synthetic corpus of the size of
test_gpu_hybrid.py's for the calls that need both stages in one index ("hyb").  Everything here is deterministic; nothing
provokes a fault: every dirtier is an input some test of the suite already runs.
"""
import ctypes as C
import functools
import os
import re

import numpy as np

import bm25_round_cases as rc
import bm25_span_cases as sc
import dense_adversary as A
import select_cases as S

MAX_QUERIES = 512            # paths for <= 64, 65 .. 128 and > 128 queries all exist; BM25 slices of 512 rows run 4 tiles per item
MAX_K = 1024
RERANK_MAX_DOCS = 1000
K_BM25 = 200
K_DENSE = 10
ALL = ("lex", "f16", "bf16", "hyb")
DENSE = ("f16", "bf16", "hyb")
SPLITS = {512: (4, 16), 16: (1, 61), 1: (1, 61)}              # BM25 rows of a slice -> (tiles per item, spans) on the lex corpus
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "modern-search-engines-project_amd", "csrc")


def _read_int(path, pattern):
    m = re.search(pattern, open(os.path.join(_CSRC, path)).read(), re.M)
    assert m, (path, pattern)
    return int(m.group(1))


@functools.lru_cache(None)
def caps():
    """The capacities the dirtiers overflow, as the library is compiled with them (read from the sources, not copied)."""
    return dict(sel_cap=_read_int("msr_internal.h", r"^#define MSR_SEL_CAP (\d+)"),
                sel_bins=_read_int("msr_internal.h", r"^#define MSR_SEL_BINS (\d+)"),
                stage=_read_int("msr_topk.hip", r"constexpr int STAGE = (\d+);"),
                gf_pair_cap=_read_int("msr_gemm_f32.hip", r"^constexpr int GF_PAIR_CAP = (\d+);"),
                gm_pair_cap=_read_int("msr_gemm.hip", r"^constexpr int GM_PAIR_CAP = (\d+);"),
                merge_cap=_read_int("msr_similar.hip", r"^constexpr int MERGE_CAP = (\d+);"),
                bt_slice=_read_int("msr_engine.hip", r"^static constexpr int BT_SLICE = (\d+);"),
                res=rc.resident_chunks())


# ------------------------------------------------------------------------------------------------------------ select cases
# dirtier -> (case of select_cases.CASES, the branch tags it is picked for); test_call_sequence_cases.py checks the tags
# against the case and, through select_cases.model, that some query of the case takes each branch
SELECT_PICKS = {
    "select_win_overflow": ("win_bin_over_cap", ("win_overflow", "row_general")),
    "select_stage_overflow_f32": ("stage_overflow_float32", ("stage_overflow",)),
    "select_stage_overflow_f64": ("stage_overflow_float64", ("stage_overflow",)),
    "select_tie_group_above_cap": ("group_float32_5000_k10", ("row_general",)),
    "select_list_ties_above_cap": ("list_ties_over_cap", ("row_general", "row_index_digit")),
    "select_fewer_valid_than_k": ("k_above_valid_float32", ("take_all",)),
    "select_within_empty_and_out_of_range": ("within_mixed_sets", ("take_all",)),
}
SELECT_PROBES = {"select_f32": "random_float32_n20000_k100", "select_f64_list": "list_nseg8"}


@functools.lru_cache(None)
def select_case(name):
    return S.build(name)


@functools.lru_cache(None)
def modelled(name):
    """-> (the SelState select_cases.model predicts for every query of the case, the branch tags the queries take)"""
    case, states, reached = select_case(name), [], set()
    for q in range(case.nq):
        _, _, st, tags = S.model(case, q)
        states.append(tuple(st))
        reached |= set(tags)
    return states, reached


@functools.lru_cache(None)
def nan_row_case():
    """Three ordinary rows of which row 1 is NaN everywhere: nothing enters its histogram, n = 0."""
    x = S.random_rows(np.float32, 3, 9000, 171)
    x[1] = np.nan
    return S.Case("all_nan_row", x, 100, set())


@functools.lru_cache(None)
def gate_per64_case():
    """test_gpu_select.py's gated case: 130 queries, a tie group above the cap in an ON slice (query 5) and in the OFF slice
    (query 70); gate words (1, 0, 5)."""
    x = S.random_rows(np.float32, 130, 9000, 71)
    x[5] = 0.5
    x[70] = 0.25
    return S.Case("gate_per64", x, 100, set())


GATE_WORDS = (1, 0, 5)


# ------------------------------------------------------------------------------------------------------------ CPU inputs
class LexInputs:
    """The 61-tile corpus and queries of bm25_span_cases.py, with test_gpu_stage1_order.py's additions (nine queries of one
    30-posting list each, one of unknown terms only) and its numpy restatement of the plan kernel's weight."""

    def __init__(self):
        self.z, self.T = sc.build_corpus()
        queries, names = sc.build_queries(self.z, self.T)
        V = len(self.z["idf"])
        for i, t in enumerate(self.T["short"]):
            queries.append([t]); names.append("short_%d" % i)
        queries.append([V + 110, -3]); names.append("unknown_only")
        self.queries, self.names = queries, names
        self.name = {n: i for i, n in enumerate(names)}
        self.df = np.diff(self.z["term_off"])
        self.tabled = set(self.T["neg_tabled"])
        self.n_docs = sc.N_DOCS
        self.mixed16 = sc.fill(43, 16).tolist()              # the probe: 16 of bm25_span_cases' own 43 queries
        self.masks = sc.within_masks()
        self.z2, _ = rc.build_corpus()                        # the rebind target: another 61-tile corpus (bm25_round_cases.py)

    def weight(self, i, ms):
        w = 0
        for t in dict.fromkeys(self.queries[i]):
            if 0 <= t < len(self.df) and self.df[t] > 0 and not (ms >= 0 and t in self.tabled and self.z["idf"][t] < 0):
                w += int(self.df[t])
        return w

    def heavy_set(self, ms, tpw):
        """-> (weights, heavy): heavy = expected postings per item above the resident chunks (msr_bm25.hip's plan kernel)."""
        w = np.array([self.weight(i, ms) for i in range(len(self.queries))])
        return w, w * tpw * sc.TILE > caps()["res"] * 64 * self.n_docs

    def slice_rows(self, kind, nq, ms=0.0):
        w, heavy = self.heavy_set(ms, SPLITS[nq][0])
        members = np.nonzero(heavy if kind == "heavy" else ~heavy)[0].tolist()
        return [members[j % len(members)] for j in range(nq)]

    def within_names(self, nq):
        names = list(self.masks)
        return [names[(r + r // len(names)) % len(names)] for r in range(nq)]


@functools.lru_cache(None)
def lex_inputs():
    return LexInputs()


class DenseInputs:
    """An adversarial corpus of dense_adversary.py and the queries of the dense entries: its planted and small-twin queries
    (ordinary: their top 10 is unambiguous or an exact tie), ten Gaussian queries, and the big twin group's query."""

    def __init__(self, fmt):
        self.c = A.build(fmt)
        c = self.c
        self.ordinary = [i for i, p in enumerate(c.queries) if p.kind != "big"]
        self.big = c.of_k(10, kinds=("big",))[0]
        rng = np.random.default_rng(7 if fmt == "f16" else 8)
        g = rng.standard_normal((10, A.DIM)).astype(np.float32) * rng.uniform(0.5, 6.0, (10, 1)).astype(np.float32)
        self.distinct = np.concatenate([c.qmat(self.ordinary), g])             # [16, 768]
        self.big_q = c.queries[self.big].q
        self.emb, self.doc_off, self.n_docs = c.emb, c.doc_off, c.n_docs
        m = lambda: np.zeros(self.n_docs, bool)
        other, block = m(), m()
        other[::2] = True
        block[c.split_doc - 200:c.split_doc + 200] = True
        self.masks = {"none": None, "empty": m(), "every_other": other, "block": block}

    def rows(self, Q, shift=0):
        """-> (index into `distinct` of every row, the matrix [Q, 768])"""
        idx = [(i * 5 + shift) % len(self.distinct) for i in range(Q)]
        return idx, self.distinct[idx]

    def within_names(self, nq):
        names = list(self.masks)
        return [names[(r + r // len(names)) % len(names)] for r in range(nq)]


@functools.lru_cache(None)
def dense_inputs(fmt):
    return DenseInputs(fmt)


class HybInputs:
    """test_gpu_hybrid.py's `hyb` fixture (the same corpus, queries and planted dense winners), with a vocabulary, a forward
    index, a facet and URLs as test_gpu_query_options.py gives them, for the text-side calls."""

    def __init__(self):
        import hybrid_ref as H
        from msretr.index import _np
        from msretr.index_build import attach_tokens
        from msretr.synthetic import synthetic_corpus, synthetic_queries
        from options_cases import _streams, _word
        from test_gpu_hybrid import DENSE_K, NH, QH, _planted, _with_urls
        ix = synthetic_corpus(NH, n_chunks=60_000, n_terms=6000, seed=31)
        terms, qv = synthetic_queries(ix, QH, seed=32, lo_rank=5, hi_rank=3000)
        qv = qv.numpy().copy()
        self.planted = _planted(ix, qv, DENSE_K, 33)
        terms = [list(t) for t in terms]
        terms[3] = [-1, -2]
        _with_urls(ix)
        ix.vocab = {_word(t): t for t in range(ix.n_terms)}
        off, tok = _streams(ix)
        attach_tokens(ix, off, tok)
        self.ix, self.terms, self.qv, self.dense_k = ix, terms, qv, DENSE_K
        self.word = _word
        self.z = {k: _np(getattr(ix, k)) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")}
        self.z["avgdl"] = ix.avgdl
        self.emb, self.doc_off, self.n_docs = _np(ix.emb), _np(ix.doc_off).astype(np.int64), ix.n_docs
        _, q200 = synthetic_queries(ix, 200, seed=52, lo_rank=5, hi_rank=3000)
        self.distinct = np.concatenate([qv, q200.numpy()[:40]])              # [64, 768]
        self.tok_off, self.tok = off, tok
        df = np.diff(self.z["term_off"])
        self.mid = [int(t) for t in np.argsort(-df, kind="stable")[100:140]]
        self.facet = np.where(np.arange(ix.n_docs) % 97 == 0, -1, np.arange(ix.n_docs) % 41).astype(np.int32)
        m = lambda: np.zeros(self.n_docs, bool)
        other, block = m(), m()
        other[::2] = True
        block[8000:8400] = True
        self.masks = {"none": None, "empty": m(), "every_other": other, "block": block}
        self.mixed16 = list(range(16))
        self.queries = terms
        self._cand = None
        self._H = H

    def rows(self, Q, shift=0):
        idx = [(i * 5 + shift) % len(self.distinct) for i in range(Q)]
        return idx, self.distinct[idx]

    def within_names(self, nq):
        names = list(self.masks)
        return [names[(r + r // len(names)) % len(names)] for r in range(nq)]

    def candidates(self):
        """The hybrid candidate lists of the 24 queries from the CPU chain (hybrid_ref.candidates), padded: the input of the
        rerank probe -> (doc int32 [Q, M], bm25 float64 [Q, M], src, n int32 [Q])."""
        if self._cand is None:
            from msretr.retriever import hybrid_k_lex
            H = self._H
            lists = [H.candidates(self.z, self.emb, self.doc_off, self.terms[q], self.qv[q], 1000, RERANK_MAX_DOCS, self.dense_k)
                     for q in range(len(self.terms))]
            self._cand = H.pad_lists(lists, hybrid_k_lex(1000, RERANK_MAX_DOCS, self.dense_k) + self.dense_k)
        return self._cand


@functools.lru_cache(None)
def hyb_inputs():
    return HybInputs()


def merge_lists_input(seed=3, G=3, Q=4, k=37):
    """Sorted per-shard lists with unique documents (test_gpu_select.py's 'alike' shape) -> (docs, scores, ns)."""
    rng = np.random.default_rng(seed)
    docs = np.full((G, Q, k), -1, np.int32); sco = np.full((G, Q, k), -np.inf, np.float32); ns = np.zeros((G, Q), np.int32)
    for g in range(G):
        for q in range(Q):
            s = rng.standard_normal(k).astype(np.float32)
            d = rng.choice(np.arange(g * 100000, (g + 1) * 100000), size=k, replace=False).astype(np.int32)
            o = np.lexsort((d, -s.astype(np.float64)))
            docs[g, q], sco[g, q], ns[g, q] = d[o], s[o], k
    return docs, sco, ns


# ------------------------------------------------------------------------------------------------------------ the bundle
def _host(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _named(names, arrays):
    return {n: a for n, a in zip(names, arrays) if a is not None}


class Bundle:
    """One engine on one index, alive for a whole test module, and the device copies of the entries' inputs."""

    def __init__(self, name, stage=None):
        import torch
        from msretr.engine import DeviceEngine
        from msretr.index import CorpusIndex
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.name, self.torch = name, torch
        self.retriever = None
        self._dev, self._sets = {}, {}
        self.stage = stage                                    # None: inputs are uploaded once and stay as they are
        self.clean = {}                                       # probe name -> its outputs as the first call after a fresh bind
        self.bf16 = name == "bf16"
        if name == "lex":
            self.inp = lex_inputs()
            self.ix = CorpusIndex(total_docs=self.inp.n_docs, **self.inp.z)
            self.ix2 = CorpusIndex(total_docs=rc.N_DOCS, **self.inp.z2)
        elif name in ("f16", "bf16"):
            self.inp = dense_inputs(name)
            self.ix = self._dense_index(CorpusIndex, self.inp.c, 0, self.inp.n_docs)
            self.ix2 = self._dense_index(CorpusIndex, self.inp.c, 0, self.inp.c.split_doc)      # the rebind target: half A
        else:
            self.inp = hyb_inputs()
            self.ix = self.inp.ix
            self.ix2 = None
        self.eng = DeviceEngine(self.ix, max_queries=MAX_QUERIES, max_k=MAX_K,
                                rerank_max_docs=RERANK_MAX_DOCS if name == "hyb" else 64)
        if self.bf16:
            self.eng.enable_bf16()
        if name == "hyb":
            from msretr.retriever import Retriever
            self.retriever = Retriever(indexer=self.eng)

    @staticmethod
    def _dense_index(CorpusIndex, c, d0, d1):
        off = c.doc_off[d0:d1 + 1] - c.doc_off[d0]
        r0, r1 = int(c.doc_off[d0]), int(c.doc_off[d1])
        return CorpusIndex(doc_ids=np.arange(d0, d1, dtype=np.int64), doc_off=off.astype(np.int32),
                           chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=c.emb[r0:r1], total_docs=c.n_docs, doc_base=d0,
                           row_base=r0)

    def fresh(self):
        """A fresh bind of the bundle's index (what the clean bytes are taken after)."""
        self.eng.rebind(self.ix)
        if self.retriever is not None:
            self.retriever._domains_bound = False

    def close(self):
        self.eng.close()

    def dev(self, key, make):
        """Device copy of an input, uploaded once."""
        if key not in self._dev:
            a = make()
            if isinstance(a, np.ndarray):
                a = self._up(a, key)
            self._dev[key] = a
        return self._dev[key]

    def docset(self, name):
        """DocSet of the inputs' mask `name` for the index that is bound now (a DocSet is tied to its index)."""
        from msretr.docset import DocSet
        key = (id(self.eng.index), name)
        if key not in self._sets:
            m = self.inp.masks[name]
            self._sets[key] = None if m is None else DocSet.from_mask(self.eng.index, m)
        return self._sets[key]

    # -- shared call helpers
    def select(self, case, key, **kw):
        d = self.dev(("select", key), lambda: {f: self._up(getattr(case, f), ("select", key, f))
                                               for f in ("scores", "idx", "counts", "win_base", "set_bits", "q_set")})
        doc, score, n, state = self.eng.debug_select(d["scores"], case.k, n=case.n, idx=d["idx"], counts=d["counts"],
                                                     seg_stride=case.seg_stride, win_base=d["win_base"], set_bits=d["set_bits"],
                                                     q_set=d["q_set"], **kw)
        doc, score, n = _host(doc, score, n)
        return dict(doc=doc, score=score, n=n, state=state.view(np.uint8).copy()), state

    def _up(self, a, key=None):
        """Host array -> device tensor.  With a stage (stream_cases.Stage: the tests on a caller's stream) the tensor is the
        stage's LIVE copy of input `key`, which the stage fills with a decoy or with `a` by device-to-device copies."""
        if a is None:
            return None
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        a = np.ascontiguousarray(a)
        if self.stage is not None:
            return self.stage.adopt(key, a)
        return self.torch.from_numpy(a).to(self.eng.device)

    def qdev(self, key, mat):
        return self.dev(("q", key), lambda: np.ascontiguousarray(mat, np.float32))


class Entry:
    """name; kind "probe" / "dirtier"; bundles it runs on; run(bundle) -> (outputs: {name: host array}, report: dict);
    check(bundle, outputs, report): the path predicate (dirtiers), raises AssertionError; methods: the DeviceEngine methods the
    entry calls; group: the dirtier group (one parametrised GPU test each); pending: split_pending expected after the call."""

    def __init__(self, name, kind, bundles, run, methods, check=None, group=None, pending=0):
        self.name, self.kind, self.bundles, self.run, self.methods = name, kind, tuple(bundles), run, tuple(methods)
        self.check, self.group, self.pending = check, group, pending

    def __repr__(self):
        return self.name


PROBES, DIRTIERS = [], []


def probe(name, bundles, methods):
    def deco(fn):
        PROBES.append(Entry(name, "probe", bundles, fn, methods))
        return fn
    return deco


def dirtier(name, group, bundles, methods, check, pending=0):
    def deco(fn):
        DIRTIERS.append(Entry(name, "dirtier", bundles, fn, methods, check=check, group=group, pending=pending))
        return fn
    return deco


def _refused(call, code=-1):
    """The call raises MsrError with `code` (MSR_ERR_INVALID) -> its message."""
    from msretr._abi import MsrError
    try:
        call()
    except MsrError as e:
        assert e.code == code, (e.code, str(e))
        return str(e)
    raise AssertionError("the call was not refused")


# ================================================================================================================= probes
for _name, _case in SELECT_PROBES.items():
    def _run(b, _name=_name, _case=_case):
        out, _ = b.select(select_case(_case), _case)
        return out, {}
    probe(_name, ALL, ("debug_select",))(_run)


@probe("merge_topk", ALL, ("merge_topk",))
def _p_merge(b):
    d, s, n = (b.dev(("merge", i), lambda a=a: a) for i, a in enumerate(merge_lists_input()))
    return _named(("doc", "score", "n"), _host(*b.eng.merge_topk(d, s, n, 37))), {}


@probe("bm25_topk_16", ("lex", "hyb"), ("bm25_topk", "pack_queries"))
def _p_bm25(b):
    q = [b.inp.queries[i] for i in b.inp.mixed16]
    return _named(("doc", "score", "n"), _host(*b.eng.bm25_topk(q, k=K_BM25))), {}


@probe("bm25_topk_within", ("lex", "hyb"), ("bm25_topk", "pack_within"))
def _p_bm25_within(b):
    q = [b.inp.queries[i] for i in b.inp.mixed16]
    sets = [b.docset(s) for s in b.inp.within_names(16)]
    return _named(("doc", "score", "n"), _host(*b.eng.bm25_topk(q, k=K_BM25, within=sets))), {}


def _dense_probe(Q):
    def run(b):
        _, q = b.inp.rows(Q)
        out = _host(*b.eng.dense_topk(b.qdev(("rows", Q), q), k=K_DENSE))
        return _named(("doc", "score", "chunk", "n"), out), dict(dense_path=b.eng.dense_path())
    return run


for _Q in (8, 100, 200):
    probe("dense_topk_%d" % _Q, DENSE, ("dense_topk", "dense_path"))(_dense_probe(_Q))


@probe("dense_topk_within", DENSE, ("dense_topk", "pack_within"))
def _p_dense_within(b):
    _, q = b.inp.rows(16, shift=1)
    sets = [b.docset(s) for s in b.inp.within_names(16)]
    out = _host(*b.eng.dense_topk(b.qdev(("rows", 16, 1), q), k=K_DENSE, within=sets))
    return _named(("doc", "score", "chunk", "n"), out), {}


def _batched_probe(Q):
    def run(b):
        _, q = b.inp.rows(Q)
        out = _host(*b.eng.dense_topk_batched(b.qdev(("rows", Q), q), k=K_DENSE))
        return _named(("doc", "score", "chunk", "n"), out), dict(batch_width=b.eng.batch_width(), gemm_ok=b.eng.batch_gemm_ok())
    return run


for _Q in (100, 200):
    probe("dense_topk_batched_%d" % _Q, ("bf16",), ("dense_topk_batched", "batch_width", "batch_gemm_ok"))(_batched_probe(_Q))

GROUP_OFF = np.array([0, 7, 8, 8, 20], np.int64)             # a group of 7 rows, one of 1, an empty one, one of 12
GROUP_EXCL = [[1, 2], [], [3], [5]]


@probe("dense_topk_grouped", DENSE, ("dense_topk_grouped",))
def _p_grouped(b):
    _, q = b.inp.rows(20, shift=2)
    out = _host(*b.eng.dense_topk_grouped(b.qdev(("rows", 20, 2), q), GROUP_OFF, GROUP_EXCL, k=K_DENSE))
    return _named(("doc", "score", "chunk", "src", "n"), out), {}


@probe("dense_begin_end", DENSE, ("dense_begin", "dense_end", "dense_split_max"))
def _p_split(b):
    _, q = b.inp.rows(100)
    assert b.eng.dense_split_max(K_DENSE) >= 100
    part = b.eng.dense_begin(b.qdev(("rows", 100), q), k=K_DENSE)
    out = _host(part, *b.eng.dense_end(100, k=K_DENSE))
    return _named(("part", "doc", "score", "chunk", "n"), out), dict(dense_path=b.eng.dense_path())


@probe("score_docs_union", ("hyb",), ("bm25_topk", "dense_topk", "bm25_score_docs", "union_candidates"))
def _p_union(b):
    i, e = b.inp, b.eng
    from msretr.retriever import hybrid_k_lex
    lex = e.bm25_topk(i.terms, k=hybrid_k_lex(1000, RERANK_MAX_DOCS, i.dense_k))
    dd, _, _, dn = e.dense_topk(b.qdev("qv", i.qv), k=i.dense_k, want_chunk=False)
    ps, pt = e.bm25_score_docs(i.terms, dd, dn)
    u = _host(*e.union_candidates(lex, dd, ps, dn))
    out = _named(("doc", "score", "src", "n"), u)
    out.update(_named(("point_score", "point_touched"), _host(ps, pt)))
    return out, {}


@probe("rerank_chain", ("hyb",), ("rerank_gather", "rerank_fuse", "diversify", "bind_doc_domains"))
def _p_rerank(b):
    i, e = b.inp, b.eng
    cd, cs, _, cn = i.candidates()
    b.retriever._ensure_response_tables()
    cos, meta = e.rerank_gather(b.qdev("qv", i.qv), cd, cn, max_chunks=10)
    fused = e.rerank_fuse(cd, cs, cn, cos, meta, smoothing=b.retriever.reranker.cfg["smoothing"], max_chunks=10)
    fin = e.diversify(fused, top_k=int(b.retriever.reranker.cfg["top_k"]),
                      diversification=bool(b.retriever.reranker.cfg.get("diversification", False)))
    out = _named(("cos", "meta"), _host(cos, meta))
    out.update(_named(("f_doc", "f_score", "f_orig", "f_chunk", "f_n", "f_rows"), _host(*fused)))
    out.update(_named(("doc", "score", "orig", "chunk", "n"), _host(*fin)))
    return out, {}


@probe("final_lists_hybrid", ("hyb",), ())
def _p_final(b):
    i = b.inp
    got = b.retriever.final_lists(i.terms, i.qv, 1000, mode="hybrid", dense_k=i.dense_k, with_source=True)
    return _named(("doc", "score", "chunk", "n", "src"), got), {}


# =============================================================================================================== dirtiers
# ---- select
def _select_dirtier(name, case_name):
    def run(b):
        out, state = b.select(select_case(case_name), case_name)
        return out, dict(state=state)

    def check(b, out, rep):
        """The exported SelState of every query is the one select_cases.model predicts (all eight fields), so the query took
        the model's branches, and the branches the dirtier is picked for are among them."""
        case, st = select_case(case_name), rep["state"]
        states, reached = modelled(case_name)
        for q in range(case.nq):
            g = tuple(int(st[q][f]) for f in S.STATE_FIELDS)
            assert g == states[q], (name, q, dict(zip(S.STATE_FIELDS, g)), dict(zip(S.STATE_FIELDS, states[q])))
            assert out["n"][q] == len(case.expected(q)[0]), (name, q)
        assert set(SELECT_PICKS[name][1]) <= reached, (name, sorted(reached))
        if name in ("select_tie_group_above_cap", "select_list_ties_above_cap", "select_win_overflow"):
            assert (st["done"] == 0).all()                    # more than MSR_SEL_CAP share the prefix: the final kernel's own loop
        elif name == "select_fewer_valid_than_k":
            assert (st["n_sel"] < case.k).all() and out["n"].tolist() == [100, 1, 0]
        elif name == "select_within_empty_and_out_of_range":  # the empty set (row 3), q_set 9 and -7 (rows 4, 5)
            assert out["n"][3:6].tolist() == [0, 0, 0] and case.q_set[3:6].tolist() == [2, 9, -7]
    dirtier(name, "select", ALL, ("debug_select",), check)(run)


for _n, (_c, _t) in SELECT_PICKS.items():
    _select_dirtier(_n, _c)


def _chk_nan(b, out, rep):
    assert out["n"].tolist() == [100, 0, 100] and (out["doc"][1] == -1).all() and rep["state"]["n_sel"][1] == 0


@dirtier("select_all_nan_row", "select", ALL, ("debug_select",), _chk_nan)
def _d_nan(b):
    out, state = b.select(nan_row_case(), "all_nan_row")
    return out, dict(state=state)


def _gate_out(b, nq, k, dt):
    t = b.torch
    return (t.full((nq, k), 12345, dtype=t.int32, device=b.eng.device), t.full((nq, k), 777.0, dtype=dt, device=b.eng.device),
            t.full((nq,), -99, dtype=t.int32, device=b.eng.device))


def _chk_gate0(b, out, rep):
    assert (out["doc"] == 12345).all() and (out["score"] == 777.0).all() and (out["n"] == -99).all()      # nothing ran


@dirtier("select_gate_word_zero", "select", ALL, ("debug_select",), _chk_gate0)
def _d_gate0(b):
    case = select_case("group_float32_5000_k10")
    gate = b.dev("gate0", lambda: np.zeros(1, np.int32))
    out, state = b.select(case, "group_float32_5000_k10", gate=gate, out=_gate_out(b, case.nq, case.k, b.torch.float32))
    return out, dict(state=state)


def _chk_gate64(b, out, rep):
    case = gate_per64_case()
    off = slice(64, 128)
    assert (out["doc"][off] == 12345).all() and (out["score"][off] == 777.0).all() and (out["n"][off] == -99).all()
    on = list(range(64)) + [128, 129]
    assert (out["n"][on] == case.k).all() and out["doc"][5].tolist() == list(range(case.k))     # the ON slice's tie group


@dirtier("select_gate_per64_mixed", "select", ALL, ("debug_select",), _chk_gate64)
def _d_gate64(b):
    case = gate_per64_case()
    gate = b.dev("gate64", lambda: np.array(GATE_WORDS, np.int32))
    out, state = b.select(case, "gate_per64", gate=gate, gate_per64=True, out=_gate_out(b, 130, case.k, b.torch.float32))
    return out, dict(state=state)


# ---- BM25
def _bm25(b, rows, k=K_BM25, ms=0.0, within=None):
    q = [b.inp.queries[i] if isinstance(i, (int, np.integer)) else i for i in rows]
    return _named(("doc", "score", "n"), _host(*b.eng.bm25_topk(q, k=k, min_score=ms, within=within)))


def _chk_unknown(b, out, rep):
    assert (out["n"] == 0).all() and (out["doc"] == -1).all() and np.isneginf(out["score"]).all()


@dirtier("bm25_unknown_and_empty_queries", "bm25", ("lex",), ("bm25_topk",), _chk_unknown)
def _d_unknown(b):
    i = b.inp
    return _bm25(b, [i.name["unknown_only"], i.name["empty"]] * 8), {}


def _chk_minus(b, out, rep):
    assert (out["score"][np.isfinite(out["score"])] < 0).any()
    assert (out["n"][12:] == K_BM25).all() and (out["score"][12:] < 0).all()      # the looked-up negative term alone: streamed


@dirtier("bm25_min_score_minus_1e9", "bm25", ("lex",), ("bm25_topk",), _chk_minus)
def _d_minus(b):
    return _bm25(b, b.inp.mixed16[:12] + [b.inp.name["neg_alone"]] * 4, ms=-1e9), {}


def _chk_k(b, out, rep):
    assert out["k1"]["doc"].shape == (16, 1) and out["kmax"]["doc"].shape == (16, MAX_K) and out["kmax"]["n"].max() == MAX_K


@dirtier("bm25_k_1_and_k_max", "bm25", ("lex",), ("bm25_topk",), _chk_k)
def _d_k(b):
    a, c = _bm25(b, b.inp.mixed16, k=1), _bm25(b, b.inp.mixed16, k=MAX_K)
    return dict(k1=a, kmax=c), {}


def _chk_split(*sizes):
    def check(b, out, rep):
        for nq in sizes:
            assert rep["split"][nq] == SPLITS[nq], (nq, rep["split"][nq])
    return check


@dirtier("bm25_max_queries_rows_then_one", "bm25", ("lex",), ("bm25_topk", "bm25_split"), _chk_split(512, 1))
def _d_max_then_one(b):
    i = b.inp
    a = _bm25(b, sc.fill(len(i.queries), MAX_QUERIES).tolist())
    c = _bm25(b, [i.name["heavy_dense"]])
    return dict(many=a, one=c), dict(split={n: b.eng.bm25_split(n) for n in (512, 1)})


@dirtier("bm25_more_rows_than_max_queries", "bm25", ("lex",), ("bm25_topk", "bm25_split"), _chk_split(512, 16))
def _d_later_slices(b):
    i = b.inp
    rows = i.slice_rows("light", 512) + i.slice_rows("heavy", 16)
    return _bm25(b, rows), dict(split={n: b.eng.bm25_split(n) for n in (512, 16)})


def _slice_dirtier(kind, nq):
    def run(b):
        return _bm25(b, b.inp.slice_rows(kind, nq)), dict(split={nq: b.eng.bm25_split(nq)})
    dirtier("bm25_every_query_%s_%d" % (kind, nq), "bm25", ("lex",), ("bm25_topk", "bm25_split"), _chk_split(nq))(run)


for _kind in ("heavy", "light"):
    for _nq in (16, 512):
        _slice_dirtier(_kind, _nq)


def _chk_empty_sets(b, out, rep):
    assert (out["n"] == 0).all()


@dirtier("bm25_within_empty_sets", "bm25", ("lex",), ("bm25_topk", "pack_within"), _chk_empty_sets)
def _d_bm25_empty(b):
    return _bm25(b, b.inp.mixed16, within=[b.docset("empty")] * 16), {}


# ---- dense, f32 rows
def _dense(b, key, q, k=K_DENSE):
    out = _host(*b.eng.dense_topk(b.qdev(key, q), k=k))
    return _named(("doc", "score", "chunk", "n"), out)


def _first_docs_with_rows(b, k):
    return np.nonzero(np.diff(b.inp.doc_off) > 0)[0][:k].tolist()


def _zero_dirtier(Q, width):
    def run(b):
        _, q = b.inp.rows(Q)
        q = q.copy()
        q[5] = 0.0
        return _dense(b, ("zero", Q), q), dict(dense_path=b.eng.dense_path(), scan_width=b.eng.scan_width())

    def check(b, out, rep):
        """The zero query ties every document at cosine 0: its entries overflow the streaming pass, the gate of its 64-query
        slice goes up and the sweeps serve that slice -- the zero query's list is the first documents in index order at 0.0,
        its neighbours' scores are the sweep's (not the bits of the pass' exact f32 finish, which `clean` holds), every other
        slice keeps the pass' bytes."""
        assert rep["dense_path"] == width and rep["scan_width"] == 256
        assert out["doc"][5].tolist() == _first_docs_with_rows(b, K_DENSE) and (out["score"][5] == 0.0).all()
        clean = b.clean.get("dense_topk_%d" % Q)
        if clean is not None:
            rest = [r for r in range(64) if r != 5]
            assert all(out[a][64:].tobytes() == clean[a][64:].tobytes() for a in ("doc", "score", "chunk", "n"))
            assert out["score"][rest].tobytes() != clean["score"][rest].tobytes(), "the gated slice holds the pass' own bits"
    dirtier("dense_zero_query_in_%d" % Q, "dense_f32", ("f16", "hyb"), ("dense_topk", "dense_path", "scan_width"), check)(run)


_zero_dirtier(100, 128)
_zero_dirtier(200, 256)


def _chk_nan_query(b, out, rep):
    assert out["n"][3] == 0 and (out["doc"][3] == -1).all() and (out["n"][[0, 1, 2, 4]] == K_DENSE).all()


@dirtier("dense_nan_query", "dense_f32", DENSE, ("dense_topk",), _chk_nan_query)
def _d_nan_query(b):
    _, q = b.inp.rows(8)
    q = q.copy()
    q[3] = np.nan
    return _dense(b, "nanq", q), {}


def _chk_twin(b, out, rep):
    """5500 documents in five levels of 1100 bit-identical rows: more than GF_PAIR_CAP entries above any threshold that keeps
    ten of them.  The answer: ten documents of the top level, ascending, one score."""
    c = b.inp.c
    assert rep["dense_path"] == 128 and 1100 * 5 > caps()["gf_pair_cap"]
    top = out["doc"][5]
    assert (np.diff(top) > 0).all() and len(set(out["score"][5].view(np.uint32).tolist())) == 1
    assert (c.row_query[c.doc_off[top]] == b.inp.big).all()
    clean = b.clean.get("dense_topk_100")
    if clean is not None:                                      # slice 1 keeps the pass' bytes; slice 0 went to the gated sweeps:
        rest = [r for r in range(64) if r != 5]               # its other rows hold the sweep's bits, not the pass' exact finish
        assert all(out[a][64:].tobytes() == clean[a][64:].tobytes() for a in ("doc", "score", "chunk", "n"))
        assert out["score"][rest].tobytes() != clean["score"][rest].tobytes(), "the gated slice holds the pass' own bits"


@dirtier("dense_twin_group_above_pair_cap", "dense_f32", ("f16",), ("dense_topk", "dense_path"), _chk_twin)
def _d_twin(b):
    _, q = b.inp.rows(100)
    q = q.copy()
    q[5] = b.inp.big_q
    return _dense(b, "twin100", q), dict(dense_path=b.eng.dense_path())


# ---- dense, bf16 image
def _raw_bf16(b, qd, Q, k):
    """msr_dense_topk_bf16 itself (dense_topk_batched reruns the overflowed queries on the host): -> out_n"""
    t, e = b.torch, b.eng
    P = lambda x: C.c_void_p(x.data_ptr())
    o = (t.empty((Q, k), dtype=t.int32, device=e.device), t.empty((Q, k), dtype=t.float32, device=e.device),
         t.empty((Q, k), dtype=t.int32, device=e.device), t.empty((Q,), dtype=t.int32, device=e.device))
    e._check(e.lib.msr_dense_topk_bf16(e.handle, P(qd), Q, k, 0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), e._stream()))
    return o[3].cpu().numpy()


def _bf16_overflow(Q):
    def run(b):
        _, q = b.inp.rows(Q)
        q = q.copy()
        q[3] = b.inp.big_q
        qd = b.qdev(("bf16big", Q), q)
        raw_n = _raw_bf16(b, qd, Q, K_DENSE)
        out = _named(("doc", "score", "chunk", "n"), _host(*b.eng.dense_topk_batched(qd, k=K_DENSE)))
        out["raw_n"] = raw_n
        return out, dict(batch_width=b.eng.batch_width(), gemm_ok=b.eng.batch_gemm_ok())

    def check(b, out, rep):
        assert rep["batch_width"] == 128 and rep["gemm_ok"] and (Q > caps()["bt_slice"]) == (Q == 200)
        assert out["raw_n"][3] == -1 and (np.delete(out["raw_n"], 3) == K_DENSE).all(), out["raw_n"][:8]
        assert out["n"][3] == K_DENSE and (np.diff(out["doc"][3]) > 0).all()       # the host's rerun: one exact tie group
    dirtier("bf16_sel_cap_overflow_%d" % Q, "dense_bf16", ("bf16",), ("dense_topk_batched", "dense_topk", "batch_width",
                                                                      "batch_gemm_ok"), check)(run)


_bf16_overflow(100)
_bf16_overflow(200)


# ---- split calls
def _begin(b):
    _, q = b.inp.rows(100)
    return b.eng.dense_begin(b.qdev(("rows", 100), q), k=K_DENSE)


def _end(b, part):
    out = _host(part, *b.eng.dense_end(100, k=K_DENSE))
    return _named(("part", "doc", "score", "chunk", "n"), out)


def _legal_while_pending(b):
    """Every call that is legal between a begin and its end -> their outputs"""
    i, e = b.inp, b.eng
    out = {}
    out["bm25"] = _named(("doc", "score", "n"), _host(*e.bm25_topk([i.queries[j] for j in i.mixed16], k=K_BM25)))
    docs = np.tile(np.arange(0, 64 * 300, 300, dtype=np.int32)[None, :], (16, 1))
    out["points"] = _named(("score", "touched"), _host(*e.bm25_score_docs([i.queries[j] for j in i.mixed16], docs)))
    _, q = i.rows(16, shift=3)
    cn = np.full(16, 64, np.int32)
    out["gather"] = _named(("cos", "meta"), _host(*e.rerank_gather(b.qdev(("rows", 16, 3), q), docs, cn, max_chunks=10)))
    d, s, n = (b.dev(("merge", j), lambda a=a: a) for j, a in enumerate(merge_lists_input()))
    out["merge"] = _named(("doc", "score", "n"), _host(*e.merge_topk(d, s, n, 37)))
    out["select"], _ = b.select(select_case("group_float32_5000_k10"), "group_float32_5000_k10")
    sets = [b.docset(s) for s in i.within_names(16)]
    out["bm25_within"] = _named(("doc", "score", "n"), _host(*e.bm25_topk([i.queries[j] for j in i.mixed16], k=K_BM25, within=sets)))
    ts = e.term_sets([[i.mid[1]], [i.mid[2]]], must_not=[[i.mid[3]], []])
    out["term_sets"] = _named(("n",), _host(e.bm25_topk([[i.mid[1], i.mid[2]]] * 2, k=50, within=ts)[2]))
    cd, cs, _, cn = i.candidates()                             # the hybrid chain behind the dense stage: union, gather, fuse, diversify
    lex = e.bm25_topk(i.terms, k=64)
    dd = b.dev("pending_dense_docs", lambda: np.ascontiguousarray(i.planted[:, :8].astype(np.int32)))
    dn = b.dev("pending_dense_n", lambda: np.full(len(i.terms), 8, np.int32))
    ps, _ = e.bm25_score_docs(i.terms, dd, dn)
    out["union"] = _named(("doc", "score", "src", "n"), _host(*e.union_candidates(lex, dd, ps, dn)))
    b.retriever._ensure_response_tables()
    cos, meta = e.rerank_gather(b.qdev("qv", i.qv), cd, cn, max_chunks=10)
    fused = e.rerank_fuse(cd, cs, cn, cos, meta, smoothing=b.retriever.reranker.cfg["smoothing"], max_chunks=10)
    fin = e.diversify(fused, top_k=int(b.retriever.reranker.cfg["top_k"]),
                      diversification=bool(b.retriever.reranker.cfg.get("diversification", False)))
    out["chain"] = _named(("doc", "score", "orig", "chunk", "n"), _host(*fin))
    return out


def _chk_split_legal(b, out, rep):
    assert rep["pending_inside"] == 100 and rep["dirty_inside"] == 0
    clean = b.clean.get("dense_begin_end")
    if clean is not None:                                      # the end's result equals the direct begin / end probe
        assert all(out["end"][a].tobytes() == clean[a].tobytes() for a in clean), "dense_end differs after the calls in between"
    for got, probe_name in (("bm25", "bm25_topk_16"), ("bm25_within", "bm25_topk_within"), ("chain", "rerank_chain")):
        if probe_name in b.clean:                              # the calls in between answer as they do with no begin pending
            assert all(out[got][a].tobytes() == b.clean[probe_name][a].tobytes() for a in out[got]), got
    assert (out["union"]["n"] >= 8).all() and out["term_sets"]["n"].sum() > 0


@dirtier("split_begin_legal_calls_end", "split", ("hyb",), ("dense_begin", "dense_end", "bm25_topk", "bm25_score_docs",
                                                            "rerank_gather", "merge_topk", "debug_select", "scratch_dirty",
                                                            "union_candidates", "rerank_fuse", "diversify", "term_sets",
                                                            "pack_within"),
         _chk_split_legal)
def _d_split_legal(b):
    part = _begin(b)
    out = _legal_while_pending(b)
    dirty = b.eng.scratch_dirty()
    out["end"] = _end(b, part)
    return out, dict(pending_inside=dirty.pop("split_pending"), dirty_inside=sum(v for v in dirty.values() if v > 0))


def _chk_split_refused(b, out, rep):
    """Every call that is refused while a begin is pending, tried in that state.  msr_dense_topk_bf16 reaches its guard only
    with the bf16 image built (NOT_BOUND otherwise): the bf16 bundle must have tried it."""
    want = {"dense_topk", "dense_topk_within", "dense_topk_grouped", "dense_begin"} | ({"dense_topk_batched"} if b.bf16 else set())
    assert set(rep["messages"]) == want and (b.name != "bf16" or "msr_dense_topk_bf16" in rep["messages"]["dense_topk_batched"])
    assert all("pending" in m or "has not been ended" in m for m in rep["messages"].values()), rep["messages"]
    assert rep["pending_inside"] == 100
    clean = b.clean.get("dense_begin_end")
    if clean is not None:
        assert all(out["end"][a].tobytes() == clean[a].tobytes() for a in clean), "dense_end differs after the refused calls"


@dirtier("split_begin_refused_calls_end", "split", DENSE, ("dense_begin", "dense_end", "dense_topk", "dense_topk_grouped",
                                                           "dense_topk_batched", "scratch_dirty"), _chk_split_refused)
def _d_split_refused(b):
    e = b.eng
    part = _begin(b)
    _, q = b.inp.rows(8)
    qd = b.qdev(("rows", 8), q)
    sets = [b.docset("every_other")] * 8
    msgs = dict(dense_topk=_refused(lambda: e.dense_topk(qd, k=K_DENSE)),
                dense_topk_within=_refused(lambda: e.dense_topk(qd, k=K_DENSE, within=sets)),
                dense_topk_grouped=_refused(lambda: e.dense_topk_grouped(qd, [0, 8], None, k=K_DENSE)),
                dense_begin=_refused(lambda: _begin(b)))
    if e._bf16:
        msgs["dense_topk_batched"] = _refused(lambda: e.dense_topk_batched(qd, k=K_DENSE))
    pending = e.scratch_dirty()["split_pending"]
    return dict(end=_end(b, part)), dict(messages=msgs, pending_inside=pending)


def _chk_split_rebind(b, out, rep):
    assert rep["pending_inside"] == 100 and rep["pending_after"] == 0 and "no matching" in rep["end_message"]


@dirtier("split_begin_then_rebind", "split", DENSE, ("dense_begin", "dense_end", "rebind", "scratch_dirty"), _chk_split_rebind)
def _d_split_rebind(b):
    _begin(b)
    inside = b.eng.scratch_dirty()["split_pending"]
    b.fresh()                                                  # the pending begin is dropped with the binding
    after = b.eng.scratch_dirty()["split_pending"]
    msg = _refused(lambda: b.eng.dense_end(100, k=K_DENSE))
    return {}, dict(pending_inside=inside, pending_after=after, end_message=msg)


# ---- refusals: one MSR_ERR_INVALID per entry point
REFUSALS_ANY = {"debug_select_k", "debug_select_nq", "merge_topk_limit", "merge_gathered_limit", "scratch_dirty_n_out"}
REFUSALS_LEX = {"bm25_topk_k", "bm25_split_0", "bm25_split_above", "bm25_score_docs_null"}
REFUSALS_DENSE = {"dense_topk_k", "dense_topk_grouped_k", "dense_begin_few", "dense_end_unmatched", "gather_rows_range",
                  "rerank_gather_width", "dense_topk_within_k"}
# the text side: the Python wrappers check sizes themselves (ValueError) before the library sees them, so these go through the
# raw ABI with a negative count, NULL arrays and every other integer -1 -- what each entry point refuses before any launch
REFUSALS_RAW = ("msr_term_sets", "msr_phrase_sets", "msr_proximity_sets", "msr_combine_sets", "msr_best_windows",
                "msr_fuzzy_terms", "msr_wildcard_terms", "msr_facet_counts", "msr_collapse_duplicates", "msr_doc_signatures")
REFUSALS_HYB = {"union_candidates_width", "rerank_fuse_width", "diversify_top_k", "bm25_topk_within_k"} | set(REFUSALS_RAW)
# Left out on purpose: the binds (msr_bind_postings / _chunks / _doc_meta / _tokens / _vocab / _facet / _signatures /
# _doc_domains, msr_enable_bf16).  A refused bind may drop the binding it was to replace (DeviceEngine.rebind: "if a bind fails
# the engine is left unbound"), so a refusal in the middle of a sequence would change what every later call sees -- by contract,
# not by a leak; the binding dirtiers cover the binds from the accepting side, test_gpu_index_edges.py, test_gpu_facets.py,
# test_gpu_dedup.py, test_gpu_fuzzy.py and test_gpu_phrase_sets.py their refusals on engines of their own.  Also left out: the
# sharded rerank exchange (EXCLUDED_METHODS) and the handle-less offline calls (index build, encoder), which own no engine.


def refusals_expected(bundle_name):
    return REFUSALS_ANY | (REFUSALS_LEX if bundle_name in ("lex", "hyb") else set()) | \
        (REFUSALS_DENSE if bundle_name in DENSE else set()) | ({"dense_topk_batched_k"} if bundle_name == "bf16" else set()) | \
        (REFUSALS_HYB if bundle_name == "hyb" else set())


def _chk_refusals(b, out, rep):
    assert set(rep["messages"]) == refusals_expected(b.name), sorted(set(rep["messages"]) ^ refusals_expected(b.name))
    assert all(rep["messages"].values()), rep["messages"]


def _raw_refused(e, name):
    """The entry point through ctypes with every pointer NULL and every number -1 -> MSR_ERR_INVALID, the message."""
    from msretr import _abi
    args = _abi._SIGNATURES[name][1]
    vals = [e.handle]
    for a in args[1:-1]:
        vals.append(-1 if a in (C.c_int, C.c_int32, C.c_int64) else a(-1.0) if a in (C.c_float, C.c_double) else None)
    rc_ = getattr(e.lib, name)(*vals, e._stream())
    msg = (e.lib.msr_last_error(e.handle) or b"").decode()
    assert rc_ == -1, (name, rc_, msg)
    return msg or name


@dirtier("refusals", "refusals", ALL, ("bm25_topk", "dense_topk", "dense_topk_batched", "debug_select", "merge_topk",
                                       "dense_topk_grouped", "dense_begin", "dense_end", "bm25_split", "bm25_score_docs",
                                       "rerank_gather", "scratch_dirty", "gather_rows", "union_candidates", "rerank_fuse",
                                       "diversify", "pack_queries", "merge_gathered", "bind_facet", "bind_signatures",
                                       "doc_signatures"), _chk_refusals)
def _d_refusals(b):
    e, t, i = b.eng, b.torch, b.inp
    m = {}
    x = b.dev("refuse_rows", lambda: np.zeros((2, 100), np.float32))
    m["debug_select_k"] = _refused(lambda: e.debug_select(x, MAX_K + 1))
    m["debug_select_nq"] = _refused(lambda: e.debug_select(t.zeros((MAX_QUERIES + 1, 8), device=e.device), 1))
    d, s, n = (t.as_tensor(a).to(e.device) for a in merge_lists_input(G=17, Q=1, k=480))
    m["merge_topk_limit"] = _refused(lambda: e.merge_topk(d, s, n, 480))
    wide = merge_lists_input(G=17, Q=1, k=480)
    ex = _Gathered(t, e.device, wide[0], wide[1], wide[2], wide[0])
    m["merge_gathered_limit"] = _refused(lambda: e.merge_gathered(ex, "doc", "score", "n", "pay", 480))
    buf = (C.c_int64 * 2)()
    rc_ = e.lib.msr_debug_scratch_dirty(e.handle, buf, 2, e._stream())
    assert rc_ == -1
    m["scratch_dirty_n_out"] = e.lib.msr_last_error(e.handle).decode()
    if b.name in ("lex", "hyb"):
        q = [i.queries[j] for j in i.mixed16]
        m["bm25_topk_k"] = _refused(lambda: e.bm25_topk(q, k=MAX_K + 1))
        m["bm25_split_0"] = _refused(lambda: e.bm25_split(0))
        m["bm25_split_above"] = _refused(lambda: e.bm25_split(MAX_QUERIES + 1))
        po, pt, pq, Q = e.pack_queries(q)
        P = lambda v: C.c_void_p(v.data_ptr())
        rc_ = e.lib.msr_bm25_score_docs(e.handle, P(po), P(pt), P(pq), Q, None, None, 4, None, None, e._stream())
        assert rc_ == -1
        m["bm25_score_docs_null"] = e.lib.msr_last_error(e.handle).decode()
    if b.name in DENSE:
        _, q8 = i.rows(8)
        qd = b.qdev(("rows", 8), q8)
        m["dense_topk_k"] = _refused(lambda: e.dense_topk(qd, k=MAX_K + 1))
        m["dense_topk_grouped_k"] = _refused(lambda: e.dense_topk_grouped(qd, [0, 8], None, k=0))
        m["dense_begin_few"] = _refused(lambda: e.dense_begin(qd, k=K_DENSE))
        m["dense_end_unmatched"] = _refused(lambda: e.dense_end(100, k=K_DENSE))
        m["gather_rows_range"] = _refused(lambda: e.gather_rows([0, int(b.eng.index.doc_off[-1])]))
        cand = np.zeros((8, e.rerank_max_docs + 1), np.int32)
        m["rerank_gather_width"] = _refused(lambda: e.rerank_gather(qd, cand, np.zeros(8, np.int32)))
        sets = [b.docset("every_other")] * 8
        m["dense_topk_within_k"] = _refused(lambda: e.dense_topk(qd, k=MAX_K + 1, within=sets))
        if e._bf16:
            m["dense_topk_batched_k"] = _refused(lambda: e.dense_topk_batched(qd, k=MAX_K + 1))
    if b.name == "hyb":
        z = lambda shape, dt: t.zeros(shape, dtype=dt, device=e.device)
        lex = (z((2, 8), t.int32), z((2, 8), t.float64), z((2,), t.int32))
        m["union_candidates_width"] = _refused(lambda: e.union_candidates(lex, z((2, 4), t.int32), z((2, 4), t.float64),
                                                                          z((2,), t.int32), max_cand=11))
        wide = e.rerank_max_docs + 1
        m["rerank_fuse_width"] = _refused(lambda: e.rerank_fuse(z((2, wide), t.int32), z((2, wide), t.float64), z((2,), t.int32),
                                                                z((2, wide, 10), t.float32), z((2, wide, 3), t.int32)))
        fused = (z((2, 8), t.int32), z((2, 8), t.float64), z((2, 8), t.float64), z((2, 8), t.int32), z((2,), t.int32))
        m["diversify_top_k"] = _refused(lambda: e.diversify(fused, top_k=0))
        m["bm25_topk_within_k"] = _refused(lambda: e.bm25_topk([[0]] * 8, k=MAX_K + 1, within=[b.docset("every_other")] * 8))
        e.bind_facet(i.facet, 41)                              # (so that facet_counts and collapse_duplicates reach their checks)
        e.bind_signatures(e.doc_signatures())
        for name in REFUSALS_RAW:
            m[name] = _raw_refused(e, name)
        assert e.has_tokens and e.has_vocab and e.has_facet and e.has_signatures
    return {}, dict(messages=m)


# ---- grouped merge and list merge
def _chk_grouped_over(b, out, rep):
    """50 copies of one row at k = 100: 5000 entries survive in one group, more than the merge's LDS image holds."""
    assert rep["entries"] == 5000 > caps()["merge_cap"]
    assert out["n"].tolist() == [100, 100] and (out["src"][0] == 0).all() and (out["src"][1] == 50).all()


@dirtier("grouped_global_record_overflow", "grouped_merge", DENSE, ("dense_topk_grouped", "dense_topk"), _chk_grouped_over)
def _d_grouped_over(b):
    _, q = b.inp.rows(1, shift=4)
    qd = b.qdev("grouped50", np.repeat(q, 55, axis=0))
    n = b.eng.dense_topk(qd[:50], k=100, want_chunk=False)[3].cpu().numpy()
    out = _host(*b.eng.dense_topk_grouped(qd, [0, 50, 55], None, k=100))
    return _named(("doc", "score", "chunk", "src", "n"), out), dict(entries=int(n.sum()))


class _Gathered:
    """The receive buffer of an all-gather (test_gpu_select.py's): `world` records of [doc | score | n | pay]."""

    def __init__(self, torch, device, docs, scores, ns, pays, lead=0):
        self.world, self.Q, k = docs.shape[:3]
        self.off, o = {}, lead
        for name, a in (("doc", docs), ("score", scores), ("n", ns), ("pay", pays)):
            self.off[name] = (o, a.dtype, a.shape[1:])
            o += (a[0].nbytes + 7) // 8 * 8
        self.record = o
        host = np.full((self.world, o), 0xA5, np.uint8)
        for name, a in (("doc", docs), ("score", scores), ("n", ns), ("pay", pays)):
            p = self.off[name][0]
            for g in range(self.world):
                host[g, p:p + a[g].nbytes] = np.ascontiguousarray(a[g]).view(np.uint8).reshape(-1)
        self.recv = torch.from_numpy(host.reshape(-1)).to(device)
        self._t = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}

    def part(self, g, name):
        o, dt, shape = self.off[name]
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        return self.recv[g * self.record + o: g * self.record + o + nb].view(self._t[np.dtype(dt)]).view(*shape)


def merge_overflow_input():
    """Lists the counting merge declines (one shard holds all of the best), invalid scores inside the counted prefix and
    counts outside [0, k]: test_gpu_select.py's 'skewed' shape and its clamped counts."""
    rng = np.random.default_rng(4)
    G, Q, k = 8, 4, 100
    docs, sco, ns = merge_lists_input(seed=5, G=G, Q=Q, k=k)
    sco[G - 1] += np.float32(8.0)
    sco[2, 0, 3] = np.nan
    sco[5, 0, k - 2:] = -np.inf
    ns[:, 2] = [-3, 0, k, k + 5, 1, -1, k + 1000, 7]
    ns[:, 3] = 0
    return docs, sco, ns, k, rng


def _chk_merge_over(b, out, rep):
    assert out["n"].tolist()[3] == 0 and out["n"][0] == 100 and out["n"][2] == 100 and (out["pay"][3] == -1).all()
    top = out["doc"][1, :100]
    assert (top >= 700000).all()                               # query 1: every winner comes from the skewed last shard


@dirtier("merge_gathered_overflow_records", "grouped_merge", ALL, ("merge_gathered",), _chk_merge_over)
def _d_merge_over(b):
    docs, sco, ns, k, _ = merge_overflow_input()
    ex = b.dev("gathered", lambda: _Gathered(b.torch, b.eng.device, docs, sco, ns, ((docs.astype(np.int64) * 7 + 3) & 0x7FFFFFFF)
                                             .astype(np.int32), 24))
    out = _host(*b.eng.merge_gathered(ex, "doc", "score", "n", "pay", k))
    return _named(("doc", "score", "n", "pay"), out), {}


# ---- binding
def _chk_rebind(b, out, rep):
    assert rep["other_docs"] != rep["docs"] or rep["other_terms"] != rep["terms"]
    assert rep["dirty_other"] == 0


@dirtier("rebind_to_a_second_index_and_back", "binding", ("lex", "f16", "bf16"), ("rebind", "bm25_topk", "dense_topk",
                                                                                   "scratch_dirty"), _chk_rebind)
def _d_rebind(b):
    e = b.eng
    rep = dict(docs=b.ix.n_docs, terms=b.ix.n_terms if b.ix.term_off is not None else 0)
    e.rebind(b.ix2)
    rep.update(other_docs=b.ix2.n_docs, other_terms=b.ix2.n_terms if b.ix2.term_off is not None else 0)
    if b.name == "lex":
        out = _named(("doc", "score", "n"), _host(*e.bm25_topk([[0, 1, 2], [5]], k=K_BM25)))
    else:
        _, q = b.inp.rows(100)
        out = _named(("doc", "score", "chunk", "n"), _host(*e.dense_topk(b.qdev(("rows", 100), q), k=K_DENSE)))
    d = e.scratch_dirty()
    d.pop("split_pending")
    rep["dirty_other"] = sum(v for v in d.values() if v > 0)
    b.fresh()
    return out, rep


def _chk_enable(b, out, rep):
    assert rep["before"]["gemm_pair_n"] == -1 and rep["after"]["gemm_pair_n"] == 0 and rep["after"]["bt_cand_n"] == 0
    assert rep["batch_width"] == 128 and rep["gemm_ok"] and (out["n"] == K_DENSE).all()


@dirtier("enable_bf16_mid_sequence", "binding", ("f16",), ("enable_bf16", "dense_topk_batched", "scratch_dirty", "rebind"), _chk_enable)
def _d_enable(b):
    e = b.eng
    before = e.scratch_dirty()
    e.enable_bf16()
    after = e.scratch_dirty()
    _, q = b.inp.rows(200)
    out = _named(("doc", "score", "chunk", "n"), _host(*e.dense_topk_batched(b.qdev(("rows", 200), q), k=K_DENSE)))
    rep = dict(before=before, after=after, batch_width=e.batch_width(), gemm_ok=e.batch_gemm_ok())
    e._bf16 = False                                            # the bundle's engine goes back to f32 rows only
    b.fresh()
    return out, rep


def _chk_binds(b, out, rep):
    assert rep["has_facet"] and rep["has_signatures"] and out["hits"][0] > 0 and out["sig"].shape == (b.inp.n_docs, 64)


@dirtier("bind_facet_signatures_domains", "binding", ("hyb",), ("bind_facet", "bind_signatures", "bind_doc_domains", "doc_signatures",
                                                                "facet_counts", "has_facet", "has_signatures"), _chk_binds)
def _d_binds(b):
    e, i = b.eng, b.inp
    e.bind_facet(i.facet, 41)
    sig = e.doc_signatures()
    e.bind_signatures(sig)
    e.bind_doc_domains(b.retriever._doc_domains())
    b.retriever._domains_bound = True
    hits, nv, tv, tc = e.facet_counts([[0], i.terms[0]], limit=10)
    return dict(hits=hits, n_values_hit=nv, top_value=tv, top_count=tc, sig=sig.cpu().numpy()), \
        dict(has_facet=e.has_facet, has_signatures=e.has_signatures)


def _chk_text(b, out, rep):
    i = b.inp
    assert out["term_n"].sum() > 0 and out["near_n"][0] >= out["phrase_n"][0] > 0
    assert (out["win_start"] >= 0).any() and rep["fuzzy"][0][0][0][0] == i.mid[1] and rep["wild"][0][1] >= 1
    assert out["hits"][0] > 0 and (out["c_n"] <= out["f_n"]).all()


@dirtier("text_side_families", "text", ("hyb",), ("term_sets", "phrase_sets", "best_windows", "fuzzy_terms", "wildcard_terms",
                                                  "facet_counts", "collapse_duplicates", "bind_facet", "bind_signatures",
                                                  "doc_signatures", "has_tokens", "has_vocab", "bm25_topk", "rerank_gather",
                                                  "rerank_fuse"), _chk_text)
def _d_text(b):
    from msretr.text import Near
    e, i = b.eng, b.inp
    assert e.has_tokens and e.has_vocab
    a, c = 30, 31                                             # frequent words with adjacent ids stand next to each other
    #                                                           (in more than half the documents: negative idf, so min_score -1e9)
    q = [[a, c], [i.mid[1], i.mid[2]]]
    out = {}
    ts = e.term_sets([[a], [i.mid[1]]], must_not=[[i.mid[3]], []])
    out["term_n"] = e.bm25_topk(q, k=50, min_score=-1e9, within=ts)[2].cpu().numpy()
    ps = e.phrase_sets([[[a, c]], []], must=[[], [i.mid[1]]])
    out["phrase_n"] = e.bm25_topk(q, k=50, min_score=-1e9, within=ps)[2].cpu().numpy()
    ns = e.phrase_sets([[Near([c, a], 3)], [Near([i.mid[1], i.mid[2]], 8, ordered=True)]])
    out["near_n"] = e.bm25_topk(q, k=50, min_score=-1e9, within=ns)[2].cpu().numpy()
    d = e.bm25_topk(q, k=8)[0].cpu().numpy()
    pair_doc = np.where(d.reshape(-1) >= 0, d.reshape(-1), 0).astype(np.int32)
    w = e.best_windows(pair_doc, np.repeat(np.arange(2, dtype=np.int32), 8), q, [[3, 2], [5, 1]], 12)
    out.update(_named(("win_start", "win_cover", "win_hits", "win_mask", "win_terms"), _host(*w)))
    word = i.word(i.mid[1])
    fz = e.fuzzy_terms([word, word[:-1] + "q" + word[-1:], "zzzzqqqq"], limit=4)
    wc = e.wildcard_terms([word[:3] + "*", "?" + word[1:]], limit=8)
    e.bind_facet(i.facet, 41)
    hits, nv, tv, tc = e.facet_counts(q, limit=10)
    out.update(hits=hits, top_value=tv, top_count=tc)
    e.bind_signatures(e.doc_signatures())
    cd, cs, _, cn = i.candidates()
    cos, meta = e.rerank_gather(b.qdev("qv", i.qv), cd, cn, max_chunks=10)
    fused = e.rerank_fuse(cd, cs, cn, cos, meta)
    kept, dropped = e.collapse_duplicates(fused, 32)
    out["f_n"], out["c_n"], out["c_doc"] = fused[4].cpu().numpy(), kept[4].cpu().numpy(), kept[0].cpu().numpy()
    return out, dict(fuzzy=fz, wild=wc)


# ---------------------------------------------------------------------------------------------------------- bookkeeping
GROUPS = ("select", "bm25", "dense_f32", "dense_bf16", "split", "refusals", "grouped_merge", "binding", "text")

# DeviceEngine's public methods that no entry calls, and why each one is not part of a call sequence
EXCLUDED_METHODS = {
    "close": "ends the engine: the bundles call it once, at the end of the module",
    "scan_arith": "a read-only report no predicate needs (test_gpu_dense_filters.py asserts it)",
    "row_copy_state": "a read-only report of what the bind built",
    "row_image_state": "a read-only report of what the bind built",
    "owned_bytes": "a read-only sum of the allocations (test_gpu_lifetime checks it across rebinds)",
    "dense_pass_info": "a diagnostic that waits for the device and reads counters the next pass rewrites",
    "rerank": "gather and fuse in one call: the rerank probe runs the two halves the live path runs",
    "rerank_gather_blocks": "sharded exchange only: the gather kernel behind it is the rerank probe's (test_gpu_multirank.py)",
    "rerank_combine": "sharded exchange only: reads and writes caller buffers, no engine scratch",
    "rerank_plan": "sharded exchange only: reads and writes caller buffers, no engine scratch",
    "rerank_gather_records": "sharded exchange only: the gather kernel behind it is the rerank probe's",
    "rerank_scatter": "sharded exchange only: reads and writes caller buffers, no engine scratch",
    "set_timing": "benchmark hook: records events, touches no scratch",
    "kernel_time_ms": "benchmark hook: reads the recorded events",
}


def entries_for(bundle_name, kind=None, group=None):
    out = []
    for e in PROBES + DIRTIERS:
        if bundle_name in e.bundles and (kind is None or e.kind == kind) and (group is None or e.group == group):
            out.append(e)
    return out


SEQUENCE_SEEDS = (101, 202, 303)
SEQUENCE_STEPS = 200


def seeded_sequence(seed, bundle_name, steps=SEQUENCE_STEPS):
    """`steps` entry names drawn from both lists for one bundle (two dirtiers for every probe, so that dirtiers meet each
    other as well); reproducible from (seed, bundle)."""
    rng = np.random.default_rng([seed, ALL.index(bundle_name)])
    p = [e.name for e in entries_for(bundle_name, "probe")]
    d = [e.name for e in entries_for(bundle_name, "dirtier")]
    out = []
    for _ in range(steps):
        pool = d if rng.random() < 2.0 / 3.0 else p
        out.append(pool[int(rng.integers(len(pool)))])
    return out


def by_name(name):
    for e in PROBES + DIRTIERS:
        if e.name == name:
            return e
    raise KeyError(name)
