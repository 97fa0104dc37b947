"""msr_collapse_duplicates (dup_matrix_kernel, collapse_resolve_kernel; DESIGN K18) where tests/test_gpu_dedup.py does not go:
exact match counts from a planted signature table at every min_matches (the early exit of the pair loop), every tile count and
an odd word count per row, leaders at slots of 512 and above, and more queries than one launch's grid takes.  Buffers, sentinel
and the exact comparison are those of test_gpu_dedup.py; the oracle is dedup_ref.collapse_lists."""
import ctypes as C

import numpy as np
import pytest
import torch

import dedup_ref as ref
from msretr.engine import DeviceEngine

pytestmark = pytest.mark.gpu
FILL = -1515870811                                           # 0xA5A5A5A5 as int32
N_TERMS = 1000
NAMES = ("doc", "score", "orig", "chunk", "n", "drop_doc", "drop_leader", "drop_matches", "drop_n")


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Collapse:
    """An engine over as many pages as `sig` has rows, with `sig` bound as its signature table."""

    def __init__(self, sig):
        rng = np.random.default_rng(3)
        self.sig, self.N = sig, len(sig)
        self.ix, _, _ = ref.index_of([rng.integers(0, N_TERMS, 3).astype(np.int32) for _ in range(self.N)], N_TERMS)
        self.eng = DeviceEngine(self.ix, max_queries=4, max_k=16, rerank_max_docs=0)
        self.eng.bind_signatures(torch.from_numpy(sig.view(np.int32)).to(self.eng.device))

    def inputs(self, doc, n, seed=1):
        """doc int32 [Q, M], n [Q] -> (doc, score descending, orig, chunk, n): values distinct per slot."""
        rng = np.random.default_rng(seed)
        Q, M = doc.shape
        return (np.ascontiguousarray(doc, np.int32), -np.sort(-rng.random((Q, M)), axis=1), rng.random((Q, M)),
                rng.integers(0, 10 ** 6, (Q, M)).astype(np.int32), np.asarray(n, np.int32))

    def run(self, ins, mm):
        """One call into buffers with one query row more than the call writes -> the nine host arrays."""
        eng, dev = self.eng, self.eng.device
        Q, M = ins[0].shape
        i32 = lambda *s: torch.full(s, FILL, dtype=torch.int32, device=dev)
        f64 = lambda *s: torch.full(s, -7.5, dtype=torch.float64, device=dev)
        outs = [i32(Q + 1, M), f64(Q + 1, M), f64(Q + 1, M), i32(Q + 1, M), i32(Q + 1), i32(Q + 1, M), i32(Q + 1, M), i32(Q + 1, M),
                i32(Q + 1)]
        need = eng.lib.msr_collapse_scratch_bytes(Q, M)
        assert need == (Q * M * ((M + 31) // 32) * 4 + 15) // 16 * 16
        scratch = torch.full((need // 8 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)      # (no memset is needed)
        dins = [torch.from_numpy(a).to(dev) for a in ins]
        rc = eng.lib.msr_collapse_duplicates(eng.handle, Q, *map(_P, dins), M, mm, *map(_P, outs), _P(scratch), need, eng._stream())
        assert rc == 0, eng.lib.msr_last_error(eng.handle)
        torch.cuda.synchronize(dev)
        assert (scratch[need // 8:] == 0x5A5A5A5A5A5A5A5A).all()                                       # nothing behind the scratch
        return [o.cpu().numpy() for o in outs]

    def want(self, ins, mm):
        return ref.collapse_lists(*ins, self.sig, mm)


def _same(got, want, Q, what):
    for g, w, name in zip(got, want, NAMES):
        if g.dtype == np.float64:
            assert (g[:Q].view(np.int64) == np.ascontiguousarray(w).view(np.int64)).all(), (what, name)
        assert (g[:Q] == w).all(), (what, name, np.argwhere(g[:Q] != w)[:4].tolist())
        tail = g[Q]                                          # the row behind the call's queries keeps the fill
        assert (tail == (-7.5 if g.dtype == np.float64 else FILL)).all(), (what, name)


@pytest.fixture(scope="module")
def planted():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    sig, rows = ref.planted_table()
    c = Collapse(sig)
    c.rows = rows
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def copies():
    """40 pages with 5 near-copies each (match counts from 64 down to a few), as test_gpu_dedup.py's lists use."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    streams, _ = ref.near_copies(40, 5, length=60, edits=30, n_terms=N_TERMS, seed=9)
    streams[7] = np.zeros(0, np.int32)
    ix, off, tok = ref.index_of(streams, N_TERMS)
    c = Collapse(ref.signatures_fast(off, tok, 4))
    yield c
    c.eng.close()


# ---- the match threshold: a pair with m matches drops iff m >= min_matches -----------------------------------------------------------
def test_planted_counts_at_every_min_matches(planted):
    M = 272                                                  # 5 tiles, 9 words per row: the last tile owns ONE word
    doc, n = ref.planted_pair_lists(planted.rows, M)
    ins = planted.inputs(doc, n)
    pairs = [planted.rows["pairs"][k] for k in sorted(planted.rows["pairs"])]
    counts = ref.pair_matches(planted.rows)
    for mm in range(1, 65):
        got = planted.run(ins, mm)
        _same(got, planted.want(ins, mm), 3, ("planted", mm))
        for q in range(3):                                   # ... and directly, without the oracle
            k = int(got[8][q])
            assert k == 2 * (65 - mm), (mm, q)
            dropped = dict(zip(got[5][q, :k].tolist(), zip(got[6][q, :k].tolist(), got[7][q, :k].tolist())))
            for (a, b), m in zip(pairs, counts):
                assert (b in dropped) == (m >= mm), (mm, q, m)
                if m >= mm:
                    assert dropped[b] == (a, m), (mm, q, m)


# ---- every tile count, odd and even word counts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 31, 32, 33, 63, 64, 65, 96, 1023, 1024])
def test_width_sweep(copies, M):
    rng = np.random.default_rng(M)
    n = [0, 1, M, M + 9, -5, max(M - 1, 0), M]
    doc = rng.integers(0, copies.N, (len(n), M)).astype(np.int32)
    doc[6] = np.arange(M) % 6                                # one group only
    doc[5, ::7] = [-1, copies.N, 7][M % 3]                   # passive slots among them
    ins = copies.inputs(doc, n, seed=M)
    dropped = 0
    for mm in ((1, 40, 58, 64) if M < 1000 else (58,)):
        got = copies.run(ins, mm)
        want = copies.want(ins, mm)
        _same(got, want, len(n), ("width", M, mm))
        assert (want[4] + want[8] == np.clip(n, 0, M)).all() and want[4][0] == 0 and want[4][4] == 0 and want[4][1] == 1
        dropped += int(want[8].sum())
    assert dropped > 0 or M == 1                             # near-copies: the lists are long enough to hold duplicates
    if M >= 1023:
        assert copies.want(ins, 58)[8][2] >= M - copies.N    # 240 pages: every later slot repeats an earlier one


# ---- the full width -----------------------------------------------------------------------------------------------------------------
def test_full_width_leaders_chain_and_passive_slots(planted):
    rows = planted.rows
    doc = np.stack([ref.full_width_list(rows, planted.N)] * 2)
    doc[1] = doc[1][::-1]                                    # the same rows in reverse: leaders and copies change places
    ins = planted.inputs(doc, [1024, 1024])
    for mm in (60, 58, 64, 1):
        got = planted.run(ins, mm)
        _same(got, planted.want(ins, mm), 2, ("full width", mm))
    got = planted.run(ins, 60)
    k = int(got[8][0])
    x, y, _ = rows["ones"]
    a, b, c = rows["chain"]
    ta, te, td = rows["two"]
    assert [got[5][0, :k].tolist(), got[6][0, :k].tolist(), got[7][0, :k].tolist()] == [[b, td, y], [a, ta, x], [61, 60, 64]]
    kept = got[0][0, :got[4][0]].tolist()
    assert got[4][0] == 1021 and c in kept and te in kept and all(int(doc[0, s]) in kept for s in (63, 64, 1023))
    assert int(np.nonzero(doc[0] == x)[0][0]) == 600 and int(np.nonzero(doc[0] == y)[0][0]) == 1000
    # reversed: the copy (slot 23) leads the row that led it (slot 423); the row at slot 33 leads both of its leaders
    k = int(got[8][1])
    assert sorted(zip(got[5][1, :k].tolist(), got[6][1, :k].tolist())) == sorted([(x, y), (ta, td), (te, td), (b, c)])


# ---- more queries than one launch of the matrix kernel takes --------------------------------------------------------------------------
def test_32770_queries(planted):
    Q = 32770
    doc = ref.many_pair_queries(planted.rows, Q)
    ins = planted.inputs(doc, np.full(Q, 2), seed=5)
    ins[4][5::11] = 1                                        # some lists hold the pair's first row only
    got = planted.run(ins, 32)
    want = planted.want(ins, 32)
    _same(got, want, Q, "32770 queries")
    assert len({tuple(r) for r in doc[32767:32770].tolist()}) == 3 and want[8][32766:32770].tolist() == [0, 0, 0, 1]
    assert 0 < want[8][:32768].sum() < 32768 and 0 < want[8][32768:].sum()
    three = tuple(np.ascontiguousarray(a[32767:32770]) for a in ins)
    alone = planted.run(three, 32)
    for g, a, name in zip(got, alone, NAMES):
        assert (np.ascontiguousarray(g[32767:32770]).view(np.uint8) == np.ascontiguousarray(a[:3]).view(np.uint8)).all(), name
