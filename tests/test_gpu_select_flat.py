"""The list rows of the exact top-k select (sel_hist_kernel / sel_compact_kernel of msr_topk.hip), which a workgroup walks FLAT:
the counts of all its segments in one go, their prefix sums in LDS, then strips of 4 x 256 element numbers mapped back to
(segment, position).  Every case goes through DeviceEngine.debug_select in list mode (f64 scores, idx, counts, seg_stride; with
and without win_base) and must equal select_cases.reference -- the plain stable sort -- exactly: n, the documents in order, the
score bits, -1 / -inf behind n.  Every call is made twice in a row (a histogram or a candidate count not left zeroed shows in
the second), and every slot of a segment past its count holds POISON: a huge finite score with a plausible document index, so
that any read past a count changes the answer.

Shapes (a list pass runs at most 4096 workgroups, 4096 / nq per query, each owning whole segments): 256 and 512 queries x 123
segments (8 and 16 segments per workgroup; 256 x 123 is the benchmark's shape), 1 / 7 / 8 / 9 / 17 segments (at 17 the
workgroups are 2 segments apart and the last ones own nothing), 1024 queries x 33 segments, and more than 2048 queries, where
ONE workgroup owns a whole row: there a workgroup's element total is what the case says (strip boundaries: 1023 / 1024 / 1025
elements in one segment, one strip and one strip + 1 over several), and 1030 segments are more than one prefix table (1024)
holds."""
import numpy as np
import pytest
import torch

import select_cases as sc
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex

pytestmark = pytest.mark.gpu

POISON = 1e300
PRIME = 4194301                                   # documents: (slot * A + B_q) mod PRIME -- distinct within a row
STRIP = 4 * 256                                   # element numbers per strip of a workgroup


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = CorpusIndex(doc_ids=np.arange(4, dtype=np.int64), doc_len=np.ones(4, np.int32), term_off=np.array([0, 1], np.int64),
                     post_doc=np.zeros(1, np.int32), post_tf=np.ones(1, np.int32), idf=np.ones(1, np.float32), avgdl=1.0,
                     total_docs=4)
    e = DeviceEngine(ix, max_queries=sc.MAX_QUERIES, max_k=1024)
    yield e
    e.close()


class ListCase:
    """counts int32 [nq, n_seg] -> poisoned rows with that many live slots at the head of each segment."""

    def __init__(self, counts, seg_stride, seed, values=None):
        rng = np.random.default_rng(seed)
        self.counts = np.ascontiguousarray(counts, np.int32)
        self.nq, self.n_seg = self.counts.shape
        self.seg_stride = int(seg_stride)
        assert (self.counts >= 0).all() and (self.counts <= self.seg_stride).all()
        stride = self.n_seg * self.seg_stride
        slot = np.arange(stride, dtype=np.int64)
        self.live = (slot % self.seg_stride)[None, :] < np.repeat(self.counts, self.seg_stride, axis=1)
        a, b = int(rng.integers(1, PRIME)), rng.integers(0, PRIME, size=(self.nq, 1))
        self.idx = ((slot[None, :] * a + b) % PRIME).astype(np.int32)        # (plausible in the poisoned slots too)
        v = np.round(np.abs(rng.standard_normal((self.nq, stride))) * 4, 2) if values is None else values
        self.scores = np.where(self.live, v, POISON)

    def win_base(self, k):
        """20-bit key prefix of the k-th score minus 2000 bins (rows with fewer than k elements: any anchor will do)."""
        wb = np.zeros(self.nq, np.uint64)
        for q in range(self.nq):
            key = np.sort(sc.ord_keys(self.scores[q, self.live[q]]))[::-1]
            if len(key):
                wb[q] = max(int(key[min(k, len(key)) - 1] >> np.uint64(sc.WIN_SHIFT)) - 2000, 0)
        return wb

    def upload(self):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        return dict(scores=t(self.scores), idx=t(self.idx), counts=t(self.counts))

    def expected(self, q, k):
        return sc.reference(self.scores[q, self.live[q]], self.idx[q, self.live[q]], k)


def _call(eng, case, dev, k, win=None, **kw):
    doc, score, n, _ = eng.debug_select(dev["scores"], k, idx=dev["idx"], counts=dev["counts"], seg_stride=case.seg_stride,
                                        win_base=win, **kw)
    return doc.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()


def _check(case, got, k, what, queries=None):
    doc, score, n = got
    for q in (range(case.nq) if queries is None else queries):
        e_doc, e_score = case.expected(q, k)
        m = len(e_doc)
        assert n[q] == m, (what, q, int(n[q]), m)
        assert doc[q, :m].tolist() == e_doc.tolist(), (what, q)
        assert sc.same_scores(score[q, :m], e_score), (what, q)
        assert (doc[q, m:] == -1).all() and np.isneginf(score[q, m:]).all(), (what, q, "padding")


def _run(eng, case, ks=(100,), wins=(False, True), what=""):
    dev = case.upload()
    for k in ks:
        for w in wins:
            win = torch.from_numpy(case.win_base(k).view(np.int64)).cuda() if w else None
            first = _call(eng, case, dev, k, win)
            second = _call(eng, case, dev, k, win)                 # straight after: hist and cand_n must have been left all zero
            _check(case, first, k, (what, k, w))
            for a, b in zip(first, second):
                assert a.tobytes() == b.tobytes(), f"{what} k={k} window={w}: the second call differs from the first"


def _random_counts(rng, nq, n_seg, seg_stride, zeros=0.25):
    c = rng.integers(0, seg_stride + 1, size=(nq, n_seg))
    c[rng.random((nq, n_seg)) < zeros] = 0
    c[rng.random((nq, n_seg)) < 0.05] = seg_stride                 # some segments full to the stride
    return c


@pytest.mark.parametrize("nq", [256, 512])
def test_123_segments_8_and_16_per_workgroup(eng, nq):
    """123 segments of 64 slots: 16 workgroups of 8 segments (the last one 3) at 256 queries -- the benchmark's shape --, 8
    workgroups of 16 (the last one 11) at 512; k = 1, 100, 1000."""
    rng = np.random.default_rng(1)
    _run(eng, ListCase(_random_counts(rng, nq, 123, 64), 64, 2), ks=(1, 100, 1000), what=f"q{nq}_nseg123")


@pytest.mark.parametrize("n_seg", [1, 7, 8, 9, 17])
def test_few_segments_and_workgroups_that_own_none(eng, n_seg):
    """256 queries: up to 16 workgroups per query.  17 segments are 2 per workgroup: workgroups 9..15 start behind the row's
    last segment (at 512 queries, 8 workgroups, the same holds for 9 segments: second half of the case)."""
    rng = np.random.default_rng(10 + n_seg)
    _run(eng, ListCase(_random_counts(rng, 256, n_seg, 64), 64, 20 + n_seg), what=f"q256_nseg{n_seg}")
    if n_seg == 9:
        _run(eng, ListCase(_random_counts(rng, 512, n_seg, 64), 64, 40), what="q512_nseg9")


def test_1024_queries_33_segments(eng):
    """4 workgroups per query: 9, 9, 9 and 6 segments."""
    rng = np.random.default_rng(3)
    _run(eng, ListCase(_random_counts(rng, 1024, 33, 16), 16, 4), what="q1024_nseg33")


def test_more_segments_than_one_prefix_table(eng):
    """2100 queries leave one workgroup per row (4096 / nq = 1): 1030 segments of 4 slots are two prefix tables, 1024 + 6
    segments, and the row's best elements sit in the second."""
    rng = np.random.default_rng(5)
    nq, n_seg = 2100, 1030
    counts = _random_counts(rng, nq, n_seg, 4, zeros=0.4)
    counts[:, 1024:] = [4, 0, 3, 4, 0, 1]
    v = np.round(np.abs(rng.standard_normal((nq, n_seg * 4))) * 4, 2)
    v[:, 1024 * 4:] += 100.0
    _run(eng, ListCase(counts, 4, 6, values=v), ks=(10,), what="q2100_nseg1030")


def _one_workgroup_rows(patterns, seg_stride):
    """2100 queries (one workgroup per row), row q takes patterns[q % len(patterns)]"""
    return np.array([patterns[q % len(patterns)] for q in range(2100)], np.int32), seg_stride


def test_count_patterns_at_the_strip_boundary(eng):
    """One workgroup per row, 4 segments of 1100 slots: a segment of 1023 / 1024 / 1025 elements (one strip is 4 x 256), a
    workgroup total of exactly one strip and of one strip + 1 over several segments, all empty, one full segment among empty
    ones, zeros between non-zeros."""
    patterns = [(1023, 0, 0, 0), (0, 1024, 0, 0), (0, 0, 0, 1025), (500, 0, 524, 0), (500, 1, 524, 0), (0, 0, 0, 0),
                (0, 0, 1100, 0), (0, 7, 0, 300), (1100, 1100, 1100, 1100), (1, 0, 0, 0), (0, 0, 0, 1), (2 * STRIP - 1100, 0, 1100, 1)]
    assert sum(patterns[3]) == STRIP and sum(patterns[4]) == STRIP + 1 and sum(patterns[-1]) == 2 * STRIP + 1
    counts, stride = _one_workgroup_rows(patterns, 1100)
    _run(eng, ListCase(counts, stride, 7), ks=(100, 1000), what="strip_boundaries")


def test_tie_group_across_two_segments(eng):
    """12 equal scores, 6 at the end of one segment and 6 at the head of the next -- inside one workgroup's range (segments 2 | 3:
    32 segments are 2 per workgroup) and across two workgroups' (15 | 16) --, 3 scores above them, k = 10 cuts the group: the
    lowest documents win."""
    nq, n_seg, ss = 256, 32, 64
    counts = np.full((nq, n_seg), 40, np.int32)
    rng = np.random.default_rng(8)
    v = rng.random((nq, n_seg * ss))
    for q in range(nq):
        a = 2 if q % 2 == 0 else 15
        v[q, a * ss + 34: a * ss + 40] = 2.0
        v[q, (a + 1) * ss: (a + 1) * ss + 6] = 2.0
        v[q, [5, 20 * ss + 1, 31 * ss + 39]] = 3.0
    case = ListCase(counts, ss, 9, values=v)
    _run(eng, case, ks=(10,), what="tie_straddles")
    e_doc, e_score = case.expected(0, 10)
    assert (e_score[:3] == 3.0).all() and (e_score[3:] == 2.0).all() and (np.diff(e_doc[3:]) > 0).all()


def test_gate_forms_off_and_on(eng):
    """One gate word for the call, and one word per 64 queries: gated-off queries keep their outputs, the others are exact."""
    rng = np.random.default_rng(11)
    case = ListCase(_random_counts(rng, 130, 24, 64), 64, 12)
    dev, k = case.upload(), 100
    fresh = lambda: (torch.full((130, k), 12345, dtype=torch.int32, device="cuda"),
                     torch.full((130, k), 777.0, dtype=torch.float64, device="cuda"),
                     torch.full((130,), -99, dtype=torch.int32, device="cuda"))
    untouched = lambda o, rows: bool((o[0][rows] == 12345).all() and (o[1][rows] == 777.0).all() and (o[2][rows] == -99).all())
    out, gate = fresh(), torch.zeros(1, dtype=torch.int32, device="cuda")
    _call(eng, case, dev, k, gate=gate, out=out)
    assert untouched(out, slice(None))
    gate.fill_(1)
    _check(case, _call(eng, case, dev, k, gate=gate, out=out), k, "gate word on")
    out, gate = fresh(), torch.tensor([1, 0, 5], dtype=torch.int32, device="cuda")
    got = _call(eng, case, dev, k, gate=gate, gate_per64=True, out=out)
    _check(case, got, k, "gate per 64", list(range(64)) + [128, 129])
    assert untouched(out, slice(64, 128))
    _check(case, _call(eng, case, dev, k), k, "ungated, straight after")
