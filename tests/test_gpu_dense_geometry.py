"""Every instance of the K-split sweep (dense_ksplit_kernel) on the document layouts of tests/dense_geometry_cases.py: the edges
of the bind rule, sustained sparse layouts, runs of chunk-less documents, one document owning every row, shards.

Per case and engine the engine's own report says which kernel ran (scan_width / scan_arith / batch_width / dense_path), and
must agree with the restated bind rule: accepted layouts take the K-split sweep, refused ones the narrow kernel (width 32) --
and both must give the oracle's answer.  Each call is checked with the project's dense parity rule (check_dense: scores within
1e-5, set differences only among scores within 2e-5, ties by ascending document) and, with k = the number of documents that
have chunks, exactly: that many results, exactly those documents, no chunk-less one, the planted document first with a score
within 1e-5 of 1.  The exact checks are the ones a ring slot shared by two documents fails."""
import numpy as np
import pytest

import dense_geometry_cases as G
from similar_ref import merge_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ("edge", "sustained", "runs", "owner", "shards")
# engine kind -> (DeviceEngine arguments, query counts, arithmetic)
KINDS = {
    "default": (dict(), (1, 32, 33, 64), "f16x2"),               # f16x2: the 8-wave (<= 32 queries) and 12-wave instances
    "exact": (dict(scan_variant=2), (40, 64), "f32"),            # exact f32 products (K-split for 33 .. 64 queries)
    "presplit": (dict(scan_variant=15), (1, 32, 33, 64), "f16x2"),   # pre-split copy of the rows
    "bf16": (dict(), (40, 64, 100, 128), "f16x2"),               # dense_topk_batched: pipelined ring of 128; ring of 64 above 64
}


@pytest.fixture(scope="module")
def mods():
    from msretr.docset import DocSet
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    from oracle import dense_ref, rerank_ref
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex, DocSet=DocSet, dense_ref=dense_ref, rerank_ref=rerank_ref,
                n_cus=torch.cuda.get_device_properties(0).multi_processor_count)


_CORPORA = {}


def corpus_of(case):
    if case.name not in _CORPORA:
        _CORPORA[case.name] = G.build(case)
    return _CORPORA[case.name]


def index_of(mods, c):
    """The case's index; a shard case goes through CorpusIndex.shard of the whole layout, rows and all."""
    n = len(c.doc_off) - 1
    mk = lambda off, emb: mods["CorpusIndex"](doc_ids=np.arange(len(off) - 1, dtype=np.int64), doc_off=off.astype(np.int32),
                                              chunk_ids=np.arange(int(off[-1]), dtype=np.int64), emb=emb,
                                              total_docs=len(off) - 1)
    if c.case.shard is None:
        return mk(c.doc_off, c.emb)
    rank, world = c.case.shard
    whole = G.BY_NAME["sustained_1x16_gap95_x64"]
    off = whole.doc_off
    b, _ = G._shard_counts(whole.counts, rank, world)
    r0 = int(off[b[rank]])
    emb = np.zeros((int(off[-1]), G.DIM), np.float32)
    emb[r0:r0 + len(c.emb)] = c.emb                          # this shard's rows in their place; the others never read
    sh = mk(off, emb).shard(rank, world)
    assert np.array_equal(np.asarray(sh.doc_off, np.int64), c.doc_off) and sh.n_docs == n
    return sh


def exact_checks(c, got, tag=""):
    """Tolerance-free: with k = the number of documents that have chunks, every query returns exactly those documents; the
    planted query (row 0 of every batch) returns its document first, at a cosine of 1."""
    doc, score, chunk, n = [x.cpu().numpy() for x in got]
    want = c.with_rows.tolist()
    for i in range(doc.shape[0]):
        assert int(n[i]) == len(want), (tag, i, int(n[i]), len(want))
        got_set = sorted(doc[i, :n[i]].tolist())
        assert got_set == want, (tag, i, sorted(set(got_set) ^ set(want))[:8])
    assert int(doc[0, 0]) == c.planted and abs(float(score[0, 0]) - 1.0) <= 1e-5, (tag, int(doc[0, 0]), float(score[0, 0]))


def serve(eng, kind, q, k):
    return eng.dense_topk_batched(q, k=k) if kind == "bf16" else eng.dense_topk(q, k=k)


def expected_report(c, kind, n_cus):
    """-> (scan_width, batch_width or None) the engine must report for this layout."""
    r = G.bind_rule(c.doc_off, n_cus=n_cus)
    return (64 if r["wide_ok"] else 32), ((128 if r["wide_ok64"] else 64) if kind == "bf16" else None)


def run_case(mods, case, kind, checks=(G.check_dense, exact_checks)):
    """One engine on one layout: the report, then every query count of the kind.  -> {query count: path reported}."""
    c = corpus_of(case)
    args, counts, arith = KINDS[kind]
    k = len(c.with_rows)
    eng = mods["DeviceEngine"](index_of(mods, c), max_queries=128, max_k=max(k, 1), rerank_max_docs=0, **args)
    try:
        width, bwidth = expected_report(c, kind, mods["n_cus"])
        if mods["n_cus"] == 256:
            assert width == (64 if case.wide[0] else 32)     # the verdict written next to the case
        assert eng.scan_arith() == arith and eng.scan_width() == width, (case.name, kind, eng.scan_arith(), eng.scan_width())
        if kind == "bf16":
            eng.enable_bf16()
            assert eng.batch_width() == bwidth, (case.name, eng.batch_width())
        paths = {}
        for Q in counts:
            if Q > 64 and bwidth != 128:
                continue                                     # the ring of 64 only serves corpora that admit it
            q = c.q[:Q]
            got = serve(eng, kind, q, k)
            if kind != "bf16":
                paths[Q] = eng.dense_path()
                # the exact-f32 K-split instance serves 33 .. 64 queries; the f16x2 ones every count
                assert paths[Q] == width, (case.name, kind, Q, paths[Q])
            tag = f"{case.name}/{kind}/Q{Q}"
            for chk in checks:
                if chk is G.check_dense:
                    chk(mods, eng, c.doc_off, c.emb, q, k, 0, got)
                else:
                    chk(c, got, tag)
        return paths
    finally:
        eng.close()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("family", FAMILIES)
def test_every_instance_on_every_layout(mods, family, kind):
    cases = [c for c in G.CASES if c.family == family]
    assert cases
    ran_wide = 0
    for case in cases:
        run_case(mods, case, kind)
        ran_wide += case.wide[0]
    if family != "shards":                                   # (the shards of the 95-gap layout are refused: narrow kernel)
        assert ran_wide > 0


def test_within_and_grouped_share_the_sweep_bit_for_bit(mods):
    """msr_dense_topk_within with a set of every document and msr_dense_topk_grouped with one group run the same sweep: the
    restricted call returns the plain call's bits, the grouped call the host merge of the plain call's lists."""
    for case in (c for c in G.CASES if c.family == "sustained"):
        c = corpus_of(case)
        ix = index_of(mods, c)
        k = len(c.with_rows)
        eng = mods["DeviceEngine"](ix, max_queries=128, max_k=k, rerank_max_docs=0)
        try:
            everything = mods["DocSet"].from_mask(ix, np.ones(len(c.doc_off) - 1, bool))
            for Q in (1, 33, 64):
                q = c.q[:Q]
                plain = [x.cpu().numpy() for x in eng.dense_topk(q, k=k)]
                path = eng.dense_path()
                assert path == eng.scan_width() == expected_report(c, "default", mods["n_cus"])[0]
                got = eng.dense_topk(q, k=k, within=everything)
                assert eng.dense_path() == path
                exact_checks(c, got, f"{case.name}/within/Q{Q}")
                for a, b in zip(plain, [x.cpu().numpy() for x in got]):
                    assert a.tobytes() == b.tobytes(), (case.name, Q)
                gd, gs, gc, gsrc, gn = [x.cpu().numpy() for x in eng.dense_topk_grouped(q, [0, Q], k=k)]
                want = merge_lists(*plain, [0, Q], [[]], k)[0]
                assert int(gn[0]) == len(want) == k
                assert [(int(gd[0, j]), gs[0, j], int(gc[0, j]), int(gsrc[0, j])) for j in range(k)] == want, (case.name, Q)
                assert sorted(gd[0].tolist()) == c.with_rows.tolist()
                assert int(gd[0, 0]) == c.planted and abs(float(gs[0, 0]) - 1.0) <= 1e-5 and int(gsrc[0, 0]) == 0
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------ random layouts, unit rows
hyp = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402

SET = settings(max_examples=25, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def random_counts(rng, n_docs, max_ch, max_run):
    """Chunk counts from a mixture: a leading and a trailing run of 0 .. 100 chunk-less documents; between them stretches of
    documents with 0 .. max_ch chunks, with one chunk each, or with max_ch / 2 .. max_ch, each stretch followed by a run of
    0 .. max_run chunk-less documents.  (The bind rule takes nearly every layout with max_run <= 12 and about a fifth of
    those with 100: both kernels get their share.)"""
    counts = [0] * int(rng.integers(0, 101))
    while len(counts) < n_docs:
        kind = rng.choice(["mixed", "ones", "full"], p=[0.4, 0.2, 0.4])
        n = int(rng.integers(1, 40))
        if kind == "mixed":
            counts += rng.integers(0, max_ch + 1, size=n).tolist()
        elif kind == "ones":
            counts += [1] * n
        else:
            counts += rng.integers(max(1, max_ch // 2), max_ch + 1, size=n).tolist()
        counts += [0] * int(rng.integers(0, max_run + 1))
    counts = counts[:n_docs]
    tail = int(rng.integers(0, 101))
    if tail < n_docs:
        counts[n_docs - tail:] = [0] * tail
    if sum(counts) == 0:
        counts[0] = 1
    return counts


@SET
@given(seed=st.integers(0, 10 ** 6), n_docs=st.integers(1, 400), max_ch=st.integers(1, 16), Q=st.sampled_from([1, 32, 33, 64]),
       k=st.sampled_from([1, 10, 100]), batched=st.booleans())
def test_dense_random_sparse_layouts_unit_rows(seed, n_docs, max_ch, Q, k, batched):
    """test_gpu_property.test_dense_random_corpora with unit rows only -- so the default f16x2 instances run, which a row of
    norm 2.5 rules out there -- up to 64 queries, and runs of chunk-less documents in the layout.  Same assertions, plus the
    engine's report against the restated bind rule.  Smaller corpora than there (the oracle runs for up to 64 queries per
    example); still up to 25 spans."""
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    from oracle import dense_ref
    rng = np.random.default_rng(seed)
    doc_off = G.offsets(random_counts(rng, n_docs, max_ch, max_run=int(rng.choice([0, 4, 12, 31, 100]))))
    emb = rng.standard_normal((int(doc_off[-1]), 768)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    ix = CorpusIndex(doc_ids=np.arange(n_docs, dtype=np.int64), doc_off=doc_off.astype(np.int32),
                     chunk_ids=np.arange(doc_off[-1], dtype=np.int64), emb=emb, total_docs=n_docs)
    eng = DeviceEngine(ix, max_queries=64, max_k=100)
    rule = G.bind_rule(doc_off, n_cus=torch.cuda.get_device_properties(0).multi_processor_count)
    # (at most 6 400 rows: too few tiles for the streaming pass, so the width is the sweep's)
    assert eng.scan_arith() == "f16x2" and eng.scan_width() == (64 if rule["wide_ok"] else 32)
    if batched:
        eng.enable_bf16()
        assert eng.batch_width() == (128 if rule["wide_ok64"] else 64)
    q = (rng.standard_normal((Q, 768)) * rng.uniform(0.1, 20)).astype(np.float32)
    fn = eng.dense_topk_batched if batched else eng.dense_topk
    doc, score, chunk, cnt = [x.cpu().numpy() for x in fn(q, k=k)]
    for i in range(Q):
        best, arg = dense_ref.doc_scores(emb, doc_off, q[i], 0)
        oi, os_, _ = dense_ref.quick_search(emb, doc_off, q[i], k, 0)
        assert cnt[i] == len(oi)
        np.testing.assert_allclose(score[i, :cnt[i]], os_, rtol=0, atol=1e-5)
        np.testing.assert_allclose(score[i, :cnt[i]], best[doc[i, :cnt[i]]], rtol=0, atol=1e-5)
        assert all(abs(best[d] - os_[-1]) <= 2e-5 for d in set(doc[i, :cnt[i]].tolist()) ^ set(oi.tolist()))
        lo, hi = doc_off[doc[i, :cnt[i]]], doc_off[doc[i, :cnt[i]] + 1]
        assert np.all((chunk[i, :cnt[i]] >= lo) & (chunk[i, :cnt[i]] < hi))
    eng.close()
