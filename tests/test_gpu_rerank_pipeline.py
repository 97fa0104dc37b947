"""The rerank stage after its rework (csrc/msr_rerank.hip): the gather's flat row pipeline and the fuse
kernel without its first sort.

Gather.  tests/golden/rerank_gather_parent.npz holds every word the gather wrote BEFORE the pipeline (recorded by
tools/record_rerank_gather.py on the parent commit): the new kernel must write the same bits -- both layouts, max_chunks 10
and 3, one wave per slot (1 and 3 queries) and one wave per 8 slots (17), a shard, and the record form.  A hand-built corpus
(rerank_pipeline_cases.edge_corpus) adds the edges a row list over a block of 8 slots creates: documents of 0, 1, 2, 3, 9,
10, 11 and 25 rows, the matrix's last row, a block without a row, blocks of exactly one row and of 80 rows, 0, 1, 7, 8, 9
and 1000 candidates, padding inside a list, slots of the other shard between owned ones.  There the cosines are checked
against float64 within rerank_cases.gather_bar (derivation: tests/test_gpu_rerank.py) and, on layout 1 with unit queries --
where the normalised query and inv_norm are known on the host -- bit for bit against the kernel's lane order restated in
NumPy float32 (rerank_pipeline_cases.lane_order_cos).

Fuse.  DeviceEngine.rerank_fuse == rerank_ref.fuse_from_gather bit for bit on the cases the group table and the
register-held rows can get wrong: every list length around a wave and the sort's powers of two, every document twice, one
URL group for all, group words 0 and 1, documents of 0, 1 and 10 rows, equal cosines, equal BM25, equal documents but for
their number, repeats whose first slot comes late in the list.
"""
import os

import numpy as np
import pytest

import rerank_cases as RC
import rerank_pipeline_cases as PC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U32 = RC.U32


@pytest.fixture(scope="module")
def mods():
    from msretr.distributed import _RerankPlan
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex, Plan=_RerankPlan)


_ENG = {}


def _engine(mods, z, tag, layout=0, d0=0, d1=None):
    key = (tag, layout, d0, d1)
    if key not in _ENG:
        e1 = z["N"] if d1 is None else d1
        r0, r1 = int(z["doc_off"][d0]), int(z["doc_off"][e1])
        ix = mods["CorpusIndex"](doc_ids=np.arange(d0, e1, dtype=np.int64),
                                 doc_off=(z["doc_off"][d0:e1 + 1] - z["doc_off"][d0]).astype(np.int32),
                                 chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=z["emb"][r0:r1], total_docs=z["N"],
                                 doc_base=d0, row_base=r0, _url_group=z["url_group"][d0:e1].copy())
        _ENG[key] = mods["DeviceEngine"](ix, device=0, max_queries=32, max_k=100, rerank_max_docs=RC.M, scan_layout=layout)
    return _ENG[key]


def teardown_module(module):
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ gather: the recorded bits
def test_gather_equals_the_recorded_parent_bit_for_bit(mods):
    z = RC.gather_corpus()
    want = np.load(os.path.join(RC.GOLDEN, "rerank_gather_parent.npz"))
    got = PC.run_recorded(z, lambda layout, d0, d1: _engine(mods, z, "main", layout, d0, d1), mods["Plan"], torch)
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]
    assert not bad, f"the gather's words differ from the recorded ones in {bad}"
    assert any(want[k].any() for k in want.files if k.startswith("records_"))


# ------------------------------------------------------------------ gather: the pipeline's edges
@pytest.fixture(scope="module")
def edge():
    z = PC.edge_corpus()
    cand, n, notes = PC.edge_lists(z["N"])
    L = len(n)
    # every list twice: 2 L queries (> 16 k slots: a wave per 8 slots), the first L alone (a wave per slot)
    z["cand"], z["n"], z["notes"] = np.concatenate([cand, cand]), np.concatenate([n, n]), notes
    z["qsel"] = np.arange(2 * L) % len(z["queries"])
    z["L"] = L
    z["c64"], z["A"] = RC.cos64(z["queries"], z["emb"])
    assert 2 * L * RC.M > 16384 >= L * RC.M
    return z


def _expected_meta(z, mc, d0=0, d1=None):
    d1 = z["N"] if d1 is None else d1
    off, cand = z["doc_off"].astype(np.int64), z["cand"]
    live = (np.arange(RC.M)[None, :] < np.minimum(z["n"], RC.M)[:, None]) & (cand >= d0) & (cand < d1)
    d = np.where(live, cand, 0)
    meta = np.zeros(cand.shape + (3,), np.int32)
    meta[..., 0] = np.where(live, np.minimum(off[d + 1] - off[d], mc), 0)
    meta[..., 1] = np.where(live, z["url_group"][d] + 2, 0)
    meta[..., 2] = np.where(live, off[d], 0)
    return meta


def _used(meta):
    return np.arange(RC.MAXC)[None, None, :] < meta[..., 0][..., None]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("mc", [10, 3])
def test_gather_edges(mods, edge, layout, mc):
    z = edge
    eng = _engine(mods, z, "edge", layout)
    q = z["queries"][z["qsel"]]
    L = z["L"]
    cos, meta = [_np(x) for x in eng.rerank_gather(q, z["cand"], z["n"], max_chunks=mc)]
    cos1, meta1 = [_np(x) for x in eng.rerank_gather(q[:L], z["cand"][:L], z["n"][:L], max_chunks=mc)]
    assert np.array_equal(meta, _expected_meta(z, mc))
    assert np.array_equal(cos1.view(np.int32), cos[:L].view(np.int32)) and np.array_equal(meta1, meta[:L])
    used = _used(meta)
    assert (cos.view(np.int32)[~used] == 0).all()                                     # +0.0 in every unused place
    qi, mi, ji = np.nonzero(used)
    r = meta[qi, mi, 2] + ji
    assert r.min() == 0 and (mc < 10 or r.max() == z["C"] - 1)                        # the matrix's first and last row were read
    if layout == 0:
        inv_rel = np.full(z["C"], 13.0 * U32)
    else:
        nrm = np.linalg.norm(z["emb"].astype(np.float64), axis=1)
        inv_rel = np.abs(_np(eng._t["inv_norm"]).astype(np.float64)[:z["C"]] * nrm - 1.0)
    c64, A = z["c64"][z["qsel"][qi], r], z["A"][z["qsel"][qi], r]
    err = np.abs(cos[qi, mi, ji].astype(np.float64) - c64)
    bar = RC.gather_bar(A, c64, inv_rel[r])
    print(f"gather edges layout {layout} max_chunks {mc}: {len(r)} cosines, largest error / bar = {np.max(err / bar):.4f}")
    assert (err <= bar).all(), f"{int((err > bar).sum())} cosines outside the bar, worst {np.max(err / bar):.3f}"
    if layout == 1:
        # the normalised query is the query (its norm is exactly 1 in any summation order) and inv_norm is the bound tensor
        inv = _np(eng._t["inv_norm"])[:z["C"]]
        lo = np.stack([PC.lane_order_cos(qv, z["emb"], inv) for qv in z["queries"]])
        want = lo[z["qsel"][qi], r]
        same = cos[qi, mi, ji].view(np.int32) == want.view(np.int32)
        assert same.all(), f"{int((~same).sum())} of {len(r)} cosines differ from the lane order restated in float32"


def test_gather_edges_between_two_owners(mods, edge):
    """Shards [0, 24) and [24, N): an owner writes the one-engine words for its slots and zeros for the others, wherever in
    a block of 8 its slots lie; the two halves OR-ed together are the one engine's output."""
    z = edge
    q = z["queries"][z["qsel"]]
    cw, mw = [_np(x) for x in _engine(mods, z, "edge", 0).rerank_gather(q, z["cand"], z["n"], max_chunks=10)]
    joined_c, joined_m = np.zeros_like(cw.view(np.int32)), np.zeros_like(mw)
    for d0, d1 in ((0, 24), (24, z["N"])):
        r0 = int(z["doc_off"][d0])
        cs, ms = [_np(x) for x in _engine(mods, z, "edge", 0, d0, d1).rerank_gather(q, z["cand"], z["n"], doc_base=d0, row_base=r0,
                                                                                    max_chunks=10)]
        assert np.array_equal(ms, _expected_meta(z, 10, d0, d1))
        mine = ms[..., 1] != 0
        assert mine.any() and (~mine).any()
        assert np.array_equal(cs.view(np.int32)[mine], cw.view(np.int32)[mine])
        assert (cs.view(np.int32)[~mine] == 0).all()
        joined_c |= cs.view(np.int32); joined_m |= ms
    assert np.array_equal(joined_c, cw.view(np.int32)) and np.array_equal(joined_m, mw)


# ------------------------------------------------------------------ fuse
def _fuse_cases():
    rng = np.random.default_rng(2024)
    out = [RC.random_case(rng, n, f"n_{n}") for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024)]
    c = RC._empty(0, name="every_document_twice")                       # second halves shuffled, other BM25 scores
    docs = rng.choice(1 << 18, 500, replace=False)
    rows = {int(d): rng.uniform(-1, 1, int(rng.integers(1, 11))) for d in docs}
    for m, d in enumerate(list(docs) + list(rng.permutation(docs))):
        RC._put(c, m, int(d), float(rng.standard_normal() * 5), rows[int(d)])
    c["n"] = 1000
    out.append(c)
    c = RC._empty(0, name="one_url_group")                              # 1000 slots, one group: one document is kept
    for m, d in enumerate(rng.choice(1 << 18, 1000, replace=False)):
        RC._put(c, m, int(d), float(rng.standard_normal()), rng.uniform(-1, 1, int(rng.integers(1, 11))), group=77)
    c["n"] = 1000
    out.append(c)
    c = RC._empty(0, name="one_url_group_minimum_without_rows")         # ... and that document has no row: nothing is kept
    for m, d in enumerate(rng.choice(np.arange(10, 1 << 18), 300, replace=False)):
        RC._put(c, m, int(d), float(rng.standard_normal()), rng.uniform(-1, 1, 3), group=77)
    RC._put(c, 300, 3, 1.0, [], group=77)
    c["n"] = 301
    out.append(c)
    c = RC._empty(0, name="group_words_0_and_1")                        # nobody owns it; owned, not in urlsDB
    for m in range(400):
        RC._put(c, m, 5 * m + 1, float(rng.standard_normal()), rng.uniform(-1, 1, int(rng.integers(1, 11))), group=m // 2)
        if m % 5 == 0:
            c["meta"][m, 1] = 0
        if m % 5 == 1:
            c["meta"][m, 1] = 1
    c["n"] = 400
    out.append(c)
    for r in (0, 1, 10):
        out.append(RC.random_case(rng, 300, f"rows_{r}", rows=(r, r), p_no_rows=0.0))
    c = RC._empty(0, name="all_cosines_equal")
    for m in range(130):
        RC._put(c, m, 3 * m + 2, float(rng.standard_normal()), np.full(int(rng.integers(1, 11)), 0.375, np.float32))
    c["n"] = 130
    out.append(c)
    c = RC._empty(0, name="all_bm25_equal")
    for m in range(130):
        RC._put(c, m, 3 * m + 2, -2.25, rng.uniform(-1, 1, int(rng.integers(1, 11))))
    c["n"] = 130
    out.append(c)
    c = RC._empty(0, name="equal_but_for_the_document")                 # pairs with identical rows and BM25: document ascending
    k = 0
    for p in range(100):
        cs, bm = rng.uniform(-1, 1, int(rng.integers(1, 11))), float(rng.standard_normal())
        hi, lo = 1000 + 2 * p + 1, 1000 + 2 * p
        for d in ((hi, lo) if p % 2 else (lo, hi)):
            RC._put(c, k, d, bm, cs); k += 1
    perm = rng.permutation(k)
    for key in ("doc", "bm", "cos", "meta"):
        c[key][:k] = c[key][:k][perm]
    c["n"] = k
    out.append(c)
    c = RC._empty(0, name="repeats_whose_first_slot_comes_late")        # filled from the back: the LAST written slot of a
    docs = rng.choice(1 << 16, 120, replace=False)                      # document is its first in the list; repeats in one
    rows = {int(d): rng.uniform(-1, 1, int(rng.integers(1, 11))) for d in docs}          # wave and across waves
    seq = [int(d) for d in docs] + [int(d) for d in rng.choice(docs, 780)]
    for m in range(len(seq) - 1, -1, -1):
        RC._put(c, m, seq[m], float(rng.standard_normal() * 10), rows[seq[m]])
    for m in (1, 2, 3, 70, 899):                                        # the same document at neighbouring and far slots
        RC._put(c, m, seq[0], float(rng.standard_normal() * 10), rows[seq[0]])
    c["n"] = len(seq)
    out.append(c)
    for c in out[12:]:
        RC._garbage(c, rng)
    return out


def test_fuse_equals_the_restatement_bit_for_bit(mods):
    z = RC.gather_corpus(n_random=20)
    eng = _engine(mods, z, "fuse")
    cases = _fuse_cases()
    assert len({c["prm"] for c in cases}) == 1
    bad = []
    for i in range(0, len(cases), 24):
        part = cases[i:i + 24]
        st = lambda k: np.stack([c[k] for c in part])
        out = eng.rerank_fuse(st("doc"), st("bm"), np.array([c["n"] for c in part], np.int32),
                              torch.as_tensor(st("cos")).to(eng.device), torch.as_tensor(st("meta")).to(eng.device),
                              smoothing=part[0]["prm"][0], max_boost=part[0]["prm"][1], max_decay=part[0]["prm"][2])
        torch.cuda.synchronize()
        o = [_np(x) for x in out]
        for j, c in enumerate(part):
            got = (o[0][j], o[1][j], o[2][j], o[3][j], int(o[4][j]), int(o[5][j]))
            if not RC.same_fuse(got, RC.fuse_ref(c)):
                bad.append(c["name"])
    assert not bad, f"fuse kernel != fuse_from_gather on {bad}"
