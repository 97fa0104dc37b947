"""The shard-only native calls at the sizes and edges a balanced three-shard run never reaches, all in one process:

  msr_rerank_plan against the numpy restatement of tests/sharded_cases.py (Q and queries_per_shard above 1024, M = 1024 and
    M < 8, 64 shards, empty shards, candidates nobody owns, cand_n of 0, 1, M and more than M);
  msr_rerank_gather_records -> all-to-all by hand -> msr_rerank_scatter on UNEQUAL shards against msr_rerank_gather of one
    engine on the whole index, bit for bit (tests/test_gpu_rerank.py pins that call to float64), with the gather running in
    one, two and three launches, and word 14 of every record checked;
  msr_dense_split_max on engines whose corpus or max_queries makes the answer differ, and the dense halves run in pieces at a
    smaller size than the engine's own, as ShardedEngine._dense does after the ranks agreed on one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharded_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def mods():
    from msretr.distributed import RECORD_WORDS, _RerankPlan
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex, Plan=_RerankPlan, W=RECORD_WORDS)


def _index(mods, doc_off, emb, d0=0, d1=None):
    """Documents [d0, d1) of the corpus (doc_off, emb) as an index that knows its place in the whole."""
    n_docs = len(doc_off) - 1
    d1 = n_docs if d1 is None else d1
    r0, r1 = int(doc_off[d0]), int(doc_off[d1])
    return mods["CorpusIndex"](doc_ids=np.arange(d0, d1, dtype=np.int64), doc_off=(doc_off[d0:d1 + 1] - r0).astype(np.int32),
                               chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=emb[r0:r1], total_docs=n_docs,
                               doc_base=d0, row_base=r0)


# ------------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def bare(mods):
    eng = mods["DeviceEngine"](mods["CorpusIndex"](doc_ids=np.arange(5, dtype=np.int64)), max_queries=4, max_k=16, rerank_max_docs=0)
    yield eng
    eng.close()


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_rerank_plan_equals_the_restatement(mods, bare, c):
    """Every my_shard of the case; the arrays are poisoned before each call (an entry the kernels skip shows); recv_off is
    defined, and compared, for this rank's queries only."""
    case = sc.make_case(*c)
    world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
    cand, cn = torch.as_tensor(case["cand"]).cuda(), torch.as_tensor(case["cand_n"]).cuda()
    bounds = torch.as_tensor(case["bounds"]).cuda()
    plan = mods["Plan"](world, Q, qps, M, "cuda")
    fields = ("counts", "send_base", "send_blk", "recv_off", "pair")
    for my in range(world):
        for f in fields:
            getattr(plan, f).fill_(-7)
        bare.rerank_plan(cand, cn, bounds, my, qps, plan)
        e = sc.expected(case, my)
        n = e["hi"] - e["lo"]
        for f in fields:
            got = getattr(plan, f).cpu().numpy()
            if f == "recv_off":
                got, ref = got[:, :n], e[f][:, :n]
            else:
                ref = e[f]
            assert got.shape == ref.shape, (my, f)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, (my, f, len(bad), bad[:3].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ gather -> exchange -> scatter
class _Shards:
    """~3000 documents of 1-13 chunks (the first 10 take part), rows of norm 0.3 .. 5, cut by hand at 10 % / 60 % / 30 % of the
    documents; one engine per shard and one on the whole index, each with the gather scratch of the smallest engine
    (max_queries = 16: launches of 128 queries) and room for 1024 candidates."""

    def __init__(self, mods):
        rng = np.random.default_rng(20)
        self.n_docs = n_docs = 3001
        n = rng.integers(1, 14, size=n_docs)
        self.doc_off = np.zeros(n_docs + 1, np.int64)
        self.doc_off[1:] = np.cumsum(n)
        C = int(self.doc_off[-1])
        emb = torch.randn((C, 768), generator=torch.Generator().manual_seed(21)).numpy()
        emb *= rng.uniform(0.3, 5.0, size=(C, 1)).astype(np.float32)
        self.cuts = [0, n_docs // 10, n_docs // 10 + 6 * n_docs // 10, n_docs]
        self.world = 3
        mk = lambda ix: mods["DeviceEngine"](ix, max_queries=16, max_k=16, rerank_max_docs=1024)
        self.shards = [_index(mods, self.doc_off, emb, self.cuts[r], self.cuts[r + 1]) for r in range(3)]
        self.engs = [mk(s) for s in self.shards]
        self.full = mk(_index(mods, self.doc_off, emb))
        self.bounds = torch.tensor(self.cuts, dtype=torch.int32).cuda()

    def close(self):
        for e in self.engs + [self.full]:
            e.close()


@pytest.fixture(scope="module")
def shards(mods):
    s = _Shards(mods)
    yield s
    s.close()


@pytest.mark.parametrize("Q,M", [(5, 1), (5, 7), (5, 9), (3, 1024), (131, 20), (257, 20)],
                         ids=lambda v: str(v))
def test_records_exchange_on_unequal_shards_equals_one_engine(mods, shards, Q, M):
    """Q = 131 / 257 on engines with max_queries = 16: the gather runs in 2 / 3 launches of 128 queries, each with its own
    offsets into send_base / send_blk -- and word 14 of a record must still be the query's number within the CALL."""
    W, world, n_docs = mods["W"], shards.world, shards.n_docs
    rng = np.random.default_rng([Q, M])
    Qs = (Q + world - 1) // world
    cand = np.stack([rng.choice(n_docs, size=M, replace=False) for _ in range(Q)]).astype(np.int32)
    cand[rng.random((Q, M)) < 0.04] = -1
    cand[rng.random((Q, M)) < 0.02] = n_docs + 3                  # nobody's
    for cut in shards.cuts[1:-1]:                                  # both sides of every cut
        cand[rng.random((Q, M)) < 0.02] = cut
        cand[rng.random((Q, M)) < 0.02] = cut - 1
    cn = rng.integers(0, M + 1, Q).astype(np.int32)
    cn[0::2] = M
    if Q > 4:
        cn[1], cn[3] = 0, 1
        cand[4, :] = rng.integers(shards.cuts[1], shards.cuts[2], M)        # one query all in the large shard
        cand[2, :] = rng.integers(shards.cuts[0], shards.cuts[1], M)        # ... and one all in the small one (repeats allowed)
    q = rng.standard_normal((Q, 768)).astype(np.float32) * 3
    cand_t, cn_t = torch.as_tensor(cand).cuda(), torch.as_tensor(cn).cuda()
    ref_cos, ref_meta = shards.full.rerank_gather(q, cand_t, cn_t)
    case = dict(world=world, Q=Q, M=M, qps=Qs, bounds=np.asarray(shards.cuts, np.int32), cand=cand, cand_n=cn)
    plans, recs = [], []
    for r, (e, s_) in enumerate(zip(shards.engs, shards.shards)):
        plan = mods["Plan"](world, Q, Qs, M, "cuda")
        e.rerank_plan(cand_t, cn_t, shards.bounds, r, Qs, plan)
        rec = torch.full((Q * M * W,), -7, dtype=torch.int32, device="cuda")
        e.rerank_gather_records(q, cand_t, cn_t, plan, rec, doc_base=s_.doc_base, row_base=s_.row_base)
        plans.append(plan); recs.append(rec)
    torch.cuda.synchronize()
    for r in range(world):
        exp = sc.expected(case, r)
        lo, hi, pair, counts = exp["lo"], exp["hi"], exp["pair"], exp["counts"]
        assert np.array_equal(plans[r].pair.cpu().numpy(), pair) and np.array_equal(plans[r].counts.cpu().numpy(), counts)
        # the sender wrote exactly its records, every one complete, and nothing behind them
        sent = recs[r].view(-1, W).cpu().numpy()
        total = int(pair[r].sum())
        assert (sent[total:] == -7).all() and (sent[:total, 15] == 0).all() and (sent[:total, 0] >= 0).all()
        assert np.array_equal(sent[:total, 14], np.repeat(np.arange(Q), counts[r]))           # word 14: the query, in order
        # what the all-to-all delivers to rank r: source g's records for r's queries, sources in order
        got = []
        for g in range(world):
            first = int(pair[g, :r].sum())
            got.append(recs[g][first * W:(first + int(pair[g, r])) * W])
        recv = torch.cat(got + [torch.full((8 * W,), -7, dtype=torch.int32, device="cuda")])
        rv = recv.view(-1, W).cpu().numpy()
        for g in range(world):
            for j in range(hi - lo):
                a = int(exp["recv_off"][g, j])
                block = rv[a:a + int(counts[g, lo + j])]
                assert (block[:, 14] == lo + j).all(), (r, g, j, block[:, 14].tolist()[:4])
                assert (block[:, 0] >= 0).all() and (block[:, 0] < M).all()
        if hi > lo:
            cos, meta = shards.engs[r].rerank_scatter(recv, plans[r], lo, hi - lo, M)
            assert torch.equal(meta, ref_meta[lo:hi]), (r, "meta")
            assert torch.equal(cos.view(torch.int32), ref_cos[lo:hi].view(torch.int32)), (r, "cos")


# ------------------------------------------------------------------------------------------------ the dense halves
def _n_tiles(doc_off):
    """Row tiles as msr_bind_chunks cuts them: at most 256 rows, cut at document boundaries."""
    tiles, start = 1, 0
    for d in range(len(doc_off) - 1):
        if doc_off[d + 1] - start > 256:
            tiles, start = tiles + 1, doc_off[d]
    return tiles


class _Dense:
    def __init__(self):
        rng = np.random.default_rng(5)
        self.n_docs = n_docs = 4450
        self.n = rng.integers(1, 9, size=n_docs)
        self.doc_off = np.zeros(n_docs + 1, np.int64)
        self.doc_off[1:] = np.cumsum(self.n)
        C = int(self.doc_off[-1])
        emb = torch.randn((C, 768), generator=torch.Generator().manual_seed(6))
        self.emb = (emb / emb.norm(dim=1, keepdim=True)).numpy()
        self.n_tiles = _n_tiles(self.doc_off)


@pytest.fixture(scope="module")
def dense():
    return _Dense()


def test_dense_split_max_follows_corpus_and_max_queries(mods, dense):
    """What makes two ranks of one run answer differently: max_queries (the cap is 128 below 256 queries, else the even number
    of 128-query groups up to 8), fewer than 2 k tiles, a document of more than 256 chunks, a row off unit norm, fewer than 64
    tiles."""
    E = mods["DeviceEngine"]
    T = dense.n_tiles
    assert 64 <= T <= 128 and dense.emb.shape[0] > 19000
    ix = _index(mods, dense.doc_off, dense.emb)
    for mq, cap in ((128, 128), (256, 256), (384, 256), (512, 512)):
        e = E(ix, max_queries=mq, max_k=64, rerank_max_docs=0)
        assert e.dense_split_max(10) == cap, (mq, cap)
        if mq == 256:                                                   # 2 k against the number of tiles
            assert e.dense_split_max(T // 2) == cap and e.dense_split_max(T // 2 + 1) == 0
            assert e.dense_split_max(65) == 0                           # (k > max_k)
        e.close()
    # one document re-cut to 257 chunks (the documents around it keep theirs): no row tiles
    n, a = dense.n.tolist(), 1000
    b, rows = a, 0
    while rows < 257:
        rows += n[b]; b += 1
    n2 = n[:a] + [257] + ([rows - 257] if rows > 257 else []) + n[b:]
    off2 = np.zeros(len(n2) + 1, np.int64); off2[1:] = np.cumsum(n2)
    assert off2[-1] == dense.doc_off[-1] and max(n2) == 257
    e = E(_index(mods, off2, dense.emb), max_queries=256, max_k=64, rerank_max_docs=0)
    assert e.dense_split_max(10) == 0
    e.close()
    # one row scaled by 3: its inverse norm is outside [0.5, 2], the corpus is swept in exact f32
    emb3 = dense.emb.copy()
    emb3[12345] *= 3.0
    e = E(_index(mods, dense.doc_off, emb3), max_queries=256, max_k=64, rerank_max_docs=0)
    assert e.dense_split_max(10) == 0
    e.close()
    # the first 4000 rows only: fewer than 64 tiles
    d1 = int(np.searchsorted(dense.doc_off, 4000, side="right") - 1)
    assert _n_tiles(dense.doc_off[:d1 + 1]) < 64
    e = E(_index(mods, dense.doc_off, dense.emb, 0, d1), max_queries=256, max_k=64, rerank_max_docs=0)
    assert e.dense_split_max(10) == 0
    e.close()


def test_dense_halves_in_pieces_below_the_engines_own_size(mods, dense):
    """An engine that takes 512 queries per pair, in a run whose ranks agreed on 128: Q = 200 goes as 128 + 72, each piece
    written into its rows of the result.  Without a bound the pieces are the plain call, bit for bit; so are they with a bound
    of -inf; a bound above every cosine leaves nothing."""
    eng = mods["DeviceEngine"](_index(mods, dense.doc_off, dense.emb), max_queries=512, max_k=64, rerank_max_docs=0)
    k, Q, agreed = 10, 200, 128
    assert eng.dense_split_max(k) == 512
    rng = np.random.default_rng(9)
    q = rng.standard_normal((Q, 768)).astype(np.float32) * rng.uniform(0.5, 12, size=(Q, 1)).astype(np.float32)
    C = dense.emb.shape[0]
    q[:80] = dense.emb[rng.integers(0, C, 80)] + 0.4 * q[:80] / np.linalg.norm(q[:80], axis=1, keepdims=True)
    q[127], q[128], q[199] = dense.emb[0] * 2.0, dense.emb[C - 1] * 0.5, dense.emb[C // 2]      # exact hits at the piece edges
    q = torch.as_tensor(q).cuda()
    ref = eng.dense_topk(q, k=k)
    assert eng.dense_path() in (128, 256)                               # the streaming pass served it
    assert int(ref[3].min()) == k

    def pieces(bound):
        res = (torch.full((Q, k), -5, dtype=torch.int32, device="cuda"), torch.full((Q, k), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((Q, k), -5, dtype=torch.int32, device="cuda"), torch.full((Q,), -5, dtype=torch.int32, device="cuda"))
        for a in range(0, Q, agreed):
            b = min(Q, a + agreed)
            part = eng.dense_begin(q[a:b], k=k, k_part=(k + 2) // 3)
            assert part.shape == (b - a,) and bool((part <= 1.0 + 1e-5).all())
            eng.dense_end(b - a, k=k, bound=None if bound is None else bound[a:b], out=tuple(t[a:b] for t in res))
        return res

    for name, bound in (("none", None), ("-inf", torch.full((Q,), -np.inf, dtype=torch.float32, device="cuda"))):
        got = pieces(bound)
        for j, (a_, b_) in enumerate(zip(got, ref)):
            a_, b_ = (a_.view(torch.int32), b_.view(torch.int32)) if a_.dtype == torch.float32 else (a_, b_)
            assert torch.equal(a_, b_), (name, j, int((a_ != b_).sum()))
    doc, score, chunk, n = pieces(torch.full((Q,), 2.0, dtype=torch.float32, device="cuda"))
    assert bool((n == 0).all()) and bool((doc == -1).all()) and bool((chunk == -1).all())
    assert bool((score == -np.inf).all())
    eng.close()
