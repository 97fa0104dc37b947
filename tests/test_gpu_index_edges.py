"""The index build, merge and compact kernels at the edges no feature test reaches (cases: tests/index_cases.py, checked on
the CPU by tests/test_index_cases.py).  Everything is integer work: every comparison is exact.

scan     msr_debug_exclusive_scan (the product exclusive_scan with the scratch size the products use) against np.cumsum at
         the level boundaries 4096 and 4096^2, with values a 32-bit intermediate would get wrong.
build    msr_build_postings through raw ctypes against index_cases.ref_build on corpora built to hit the chunk, radix-block,
         pass-count and scan-level edges exactly; its sizing and refusal contract.
merge /  msr_merge_postings / msr_compact_postings with posting arrays 4, 8 and 12 bytes off a 16-byte boundary -- the scalar
compact  instantiations, chosen from the pointers' alignment alone, which the asserts on data_ptr() pin -- against the CPU
         restatement AND the aligned GPU call, with guard elements around every misaligned output."""
import ctypes as C

import numpy as np
import pytest
import torch

import index_cases as ic
from msretr import _abi
from msretr.index_build import compact_postings, merge_postings

pytestmark = pytest.mark.gpu
GUARD = -7
DEV = "cuda"


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- scan
B = ic.SCAN_BLOCK
SCAN_SIZES = (0, 1, 4, B - 1, B, B + 1, 2 * B + 1, B * B - 1, B * B, B * B + 1)


def _scan(values, with_total):
    """-> (out with 16 sentinel elements behind n, total or None)."""
    lib = _abi.load()
    n = len(values)
    src = torch.as_tensor(values).to(DEV)
    out = torch.full((n + 16,), GUARD, dtype=torch.int64, device=DEV)
    total = torch.full((1,), GUARD, dtype=torch.int64, device=DEV) if with_total else None
    rc = lib.msr_debug_exclusive_scan(_ptr(src), n, _ptr(out), _ptr(total), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.msr_last_error(None)
    return out.cpu().numpy(), None if total is None else int(total.item())


def _check_scan(values, with_total):
    values = np.asarray(values, np.int64)
    n = len(values)
    inc = np.cumsum(values, dtype=np.int64)
    want = np.concatenate([[0], inc[:-1]]) if n else inc
    out, total = _scan(values, with_total)
    assert np.array_equal(out[n:], np.full(16, GUARD)), "elements past n were written"
    bad = np.nonzero(out[:n] != want)[0]
    assert len(bad) == 0, f"n={n}: {len(bad)} wrong, first at {bad[0]}: {out[bad[0]]} != {want[bad[0]]}"
    if with_total:
        assert total == (int(inc[-1]) if n else 0)


@pytest.mark.parametrize("with_total", [True, False])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_at_its_level_boundaries(n, with_total):
    """Values from [0, 2^33): a partial sum held in 32 bits at any level is wrong; the largest total stays below 2^57."""
    assert ic.constants()["MSR_SCAN_BLOCK"] == B
    _check_scan(np.random.default_rng(n % 1000 + 5).integers(0, 1 << 33, n), with_total)


@pytest.mark.parametrize("value", [1, 0])
def test_exclusive_scan_of_ones_and_of_zeros_over_three_levels(value):
    _check_scan(np.full(B * B + 1, value, np.int64), True)
    _check_scan(np.full(2 * B + 1, value, np.int64), False)


def test_exclusive_scan_refuses_a_negative_size_and_null_arrays():
    lib = _abi.load()
    x = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert lib.msr_debug_exclusive_scan(_ptr(x), -1, _ptr(x), None, _stream()) == -1
    assert lib.msr_debug_exclusive_scan(None, 4, _ptr(x), None, _stream()) == -1
    assert lib.msr_debug_exclusive_scan(_ptr(x), 4, None, None, _stream()) == -1
    assert b"msr_debug_exclusive_scan" in lib.msr_last_error(None)


# ---------------------------------------------------------------------------------------------------------------- build
def _raw_build(tok_off, tok_ids, n_terms, capacity, slack=5):
    """msr_build_postings with caller-owned outputs pre-filled with -7 (posting arrays: capacity + slack elements)
    -> (rc, n_postings, term_off, post_doc, post_tf)."""
    lib = _abi.load()
    off = torch.as_tensor(np.asarray(tok_off, np.int64)).to(DEV)
    tok = torch.as_tensor(np.asarray(tok_ids, np.int32)).to(DEV)
    term_off = torch.full((n_terms + 1,), GUARD, dtype=torch.int64, device=DEV)
    post_doc = torch.full((capacity + slack,), GUARD, dtype=torch.int32, device=DEV)
    post_tf = torch.full((capacity + slack,), GUARD, dtype=torch.int32, device=DEV)
    n = C.c_int64(-1)
    rc = lib.msr_build_postings(_ptr(off), _ptr(tok), len(tok_off) - 1, n_terms, _ptr(term_off), _ptr(post_doc), _ptr(post_tf),
                                capacity, C.byref(n), _stream())
    torch.cuda.synchronize()
    return rc, n.value, term_off.cpu().numpy(), post_doc.cpu().numpy(), post_tf.cpu().numpy()


def _ascends_inside_terms(term_off, post_doc):
    P = int(term_off[-1])
    starts = np.zeros(P + 1, bool)
    starts[term_off] = True
    return bool((np.diff(post_doc[:P].astype(np.int64)) > 0)[~starts[1:P]].all())


def _check_build(case):
    want = ic.ref_build(case.tok_off, case.tok_ids, case.n_terms)
    P = int(want[0][-1])
    assert P == case.p_post
    rc, n, term_off, post_doc, post_tf = _raw_build(case.tok_off, case.tok_ids, case.n_terms, P)
    assert rc == 0 and n == P, (case.name, rc, n, P)
    assert np.array_equal(term_off, want[0]), (case.name, "term_off")
    assert np.array_equal(post_doc[:P], want[1]), (case.name, "post_doc")
    assert np.array_equal(post_tf[:P], want[2]), (case.name, "post_tf")
    assert (post_doc[P:] == GUARD).all() and (post_tf[P:] == GUARD).all(), (case.name, "written past P")
    assert _ascends_inside_terms(term_off, post_doc), (case.name, "documents do not ascend inside a term")


@pytest.mark.parametrize("name", [n for n, _ in ic.small_build_cases()])
def test_build_equals_the_numpy_reference_at_every_edge(name):
    c = ic.constants()
    assert (c["CH"], c["RB"]) == (ic.CH, ic.RB)
    _check_build(dict(ic.small_build_cases())[name]())


def test_build_at_scale_runs_the_keep_flag_scan_at_three_levels():
    case = ic.scale_corpus()
    assert case.p_post > B * B and case.split
    _check_build(case)


@pytest.mark.parametrize("name", ["radix_P4097_whole", "chunk_edges"])
def test_build_sizing_and_refusal_contract(name):
    """capacity 0 reports the exact count -- after the chunk merge when a document is split -- and writes no posting;
    capacity P - 1 refuses, reports P and writes no posting; capacity P succeeds.  (term_off is unspecified on the first two.)"""
    case = dict(ic.small_build_cases())[name]()
    assert case.split == (name == "chunk_edges") and (case.p_pre > case.p_post) == case.split
    P = case.p_post
    lib = _abi.load()
    rc, n, _, post_doc, post_tf = _raw_build(case.tok_off, case.tok_ids, case.n_terms, 0, slack=P + 5)
    assert rc == 0 and n == P and (post_doc == GUARD).all() and (post_tf == GUARD).all()
    rc, n, _, post_doc, post_tf = _raw_build(case.tok_off, case.tok_ids, case.n_terms, P - 1, slack=6)
    assert rc == -1 and n == P and (post_doc == GUARD).all() and (post_tf == GUARD).all()
    assert b"capacity" in lib.msr_last_error(None)
    rc, n, term_off, post_doc, post_tf = _raw_build(case.tok_off, case.tok_ids, case.n_terms, P, slack=0)
    want = ic.ref_build(case.tok_off, case.tok_ids, case.n_terms)
    assert rc == 0 and n == P
    assert np.array_equal(term_off, want[0]) and np.array_equal(post_doc, want[1]) and np.array_equal(post_tf, want[2])


def test_build_of_a_corpus_without_tokens():
    for capacity in (0, 3):
        rc, n, term_off, post_doc, post_tf = _raw_build(np.zeros(6, np.int64), np.zeros(0, np.int32), 77, capacity)
        assert rc == 0 and n == 0 and not term_off.any() and (post_doc == GUARD).all() and (post_tf == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------- placement
class _Placed:
    """An int32 array `shift` elements into a 16-byte aligned allocation filled with -7, with 8 more guard elements behind."""

    def __init__(self, n, shift, values=None):
        self.buf = torch.full((n + shift + 8,), GUARD, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.n, self.shift = n, shift
        self.view = self.buf[shift:shift + n]
        if values is not None:
            self.view.copy_(torch.as_tensor(np.asarray(values, np.int32)))
        assert self.view.data_ptr() % 16 == (4 * shift) % 16

    def guards_untouched(self, used=None):
        """Everything of the allocation outside the first `used` (default: all n) elements of the array is still -7."""
        used = self.n if used is None else used
        b = self.buf.cpu()
        return bool((b[:self.shift] == GUARD).all()) and bool((b[self.shift + used:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------------------- merge
MERGE_ARRAYS = ("a_doc", "a_tf", "b_doc", "b_tf", "post_doc", "post_tf")
MERGE_VARIANTS = {"all": dict.fromkeys(MERGE_ARRAYS, 1), "outputs": dict(post_doc=1, post_tf=1), "b_doc": dict(b_doc=1)}


def _raw_merge(a, a_map, b, b_map, n_terms, n_docs, a_docs, shifts, capacity=None):
    """msr_merge_postings with every posting array placed shifts[name] elements off 16-byte alignment
    -> (rc, term_off, post_doc, post_tf, placed outputs)."""
    lib = _abi.load()
    t = lambda x, dt: None if x is None else torch.as_tensor(np.asarray(x)).to(DEV, dt).contiguous()
    P = int(a[0][-1] + b[0][-1])
    capacity = P if capacity is None else capacity
    s = lambda name: shifts.get(name, 0)
    ad, at = _Placed(len(a[1]), s("a_doc"), a[1]), _Placed(len(a[2]), s("a_tf"), a[2])
    bd, bt = _Placed(len(b[1]), s("b_doc"), b[1]), _Placed(len(b[2]), s("b_tf"), b[2])
    od, of = _Placed(max(capacity, 1), s("post_doc")), _Placed(max(capacity, 1), s("post_tf"))
    placed = dict(a_doc=ad, a_tf=at, b_doc=bd, b_tf=bt, post_doc=od, post_tf=of)
    for name in MERGE_ARRAYS:                                 # the instantiation is a pure function of these alignments
        assert (placed[name].view.data_ptr() % 16 != 0) == (s(name) % 4 != 0), name
    ao, bo, am, bm = t(a[0], torch.int64), t(b[0], torch.int64), t(a_map, torch.int32), t(b_map, torch.int32)
    term_off = torch.full((n_terms + 1,), GUARD, dtype=torch.int64, device=DEV)
    rc = lib.msr_merge_postings(_ptr(ao), len(a[0]) - 1, _ptr(ad.view), _ptr(at.view), _ptr(am), a_docs, _ptr(bo), len(b[0]) - 1,
                                _ptr(bd.view), _ptr(bt.view), _ptr(bm), len(b_map), n_terms, n_docs, _ptr(term_off), _ptr(od.view),
                                _ptr(of.view), capacity, _stream())
    torch.cuda.synchronize()
    return rc, term_off.cpu(), od.view.cpu(), of.view.cpu(), (od, of)


def _check_scalar_merge(case, variants):
    a, a_map, b, b_map, n_terms, n_docs, a_docs = case
    want = merge_postings(*a, a_map, *b, b_map, n_terms, n_docs, a_docs=a_docs)
    P = int(want[0][-1])
    rc, *aligned, outs = _raw_merge(*case, {})
    assert rc == 0 and all(o.guards_untouched(P) for o in outs)
    for g, w in zip(aligned, want):
        assert g.dtype == w.dtype and torch.equal(g[:len(w)], w)
    for name, shifts in variants.items():
        assert any(v % 4 for v in shifts.values())           # at least one array off alignment: the scalar instantiation
        rc, *got, outs = _raw_merge(*case, shifts)
        assert rc == 0, (name, _abi.load().msr_last_error(None))
        for g, w, al in zip(got, want, aligned):
            assert torch.equal(g[:len(w)], w) and torch.equal(g, al), name
        assert all(o.guards_untouched(P) for o in outs), (name, "guard elements written")


@pytest.mark.parametrize("P", ic.MERGE_EDGE_P)
@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_scalar_merge_tile_edges(P, pattern):
    assert ic.constants()["MERGE_TILE"] == ic.MERGE_TILE
    _check_scalar_merge(ic.merge_edge_case(P, pattern), MERGE_VARIANTS)


def test_scalar_merge_at_byte_offsets_8_and_12():
    case = ic.merge_edge_case(2 * ic.MERGE_TILE + 1, "interleaved")
    _check_scalar_merge(case, {f"all+{4 * k}": dict.fromkeys(MERGE_ARRAYS, k) for k in (2, 3)} |
                        {"mixed": dict(a_doc=1, a_tf=2, b_doc=3, b_tf=0, post_doc=2, post_tf=3)})


@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_scalar_merge_head_term_and_one_sided_terms(pattern):
    _check_scalar_merge(ic.merge_head_case(pattern), MERGE_VARIANTS)


def test_scalar_merge_many_one_posting_terms():
    _check_scalar_merge(ic.merge_one_posting_case(), MERGE_VARIANTS)


# ---------------------------------------------------------------------------------------------------------------- compact
COMPACT_ARRAYS = ("post_doc", "post_tf", "out_doc", "out_tf")
COMPACT_VARIANTS = {"all": dict.fromkeys(COMPACT_ARRAYS, 1), "outputs": dict(out_doc=1, out_tf=1), "post_doc": dict(post_doc=1)}


def _raw_compact(t, keep, shifts, capacity=None):
    """msr_compact_postings with every posting array placed shifts[name] elements off 16-byte alignment
    -> (rc, n_postings, out_term_off, out_doc, out_tf, placed outputs)."""
    lib = _abi.load()
    n_terms, P = len(t[0]) - 1, int(t[0][-1])
    capacity = P if capacity is None else capacity
    s = lambda name: shifts.get(name, 0)
    pd, pt = _Placed(len(t[1]), s("post_doc"), t[1]), _Placed(len(t[2]), s("post_tf"), t[2])
    od, of = _Placed(max(capacity, 1), s("out_doc")), _Placed(max(capacity, 1), s("out_tf"))
    placed = dict(post_doc=pd, post_tf=pt, out_doc=od, out_tf=of)
    for name in COMPACT_ARRAYS:
        assert (placed[name].view.data_ptr() % 16 != 0) == (s(name) % 4 != 0), name
    off = torch.as_tensor(np.asarray(t[0], np.int64)).to(DEV)
    kp = torch.as_tensor(np.asarray(keep, np.uint8)).to(DEV)
    out_off = torch.full((n_terms + 1,), GUARD, dtype=torch.int64, device=DEV)
    n = C.c_int64(-1)
    rc = lib.msr_compact_postings(_ptr(off), n_terms, _ptr(pd.view), _ptr(pt.view), _ptr(kp), len(keep), _ptr(out_off), _ptr(od.view),
                                  _ptr(of.view), capacity, C.byref(n), _stream())
    torch.cuda.synchronize()
    return rc, n.value, out_off.cpu(), od.view.cpu(), of.view.cpu(), (od, of)


def _check_scalar_compact(t, keep, variants):
    want = compact_postings(*t, keep)
    K = int(want[0][-1])
    rc, n, *aligned, outs = _raw_compact(t, keep, {})
    assert rc == 0 and n == K and all(o.guards_untouched(K) for o in outs)
    assert torch.equal(aligned[0], want[0]) and torch.equal(aligned[1][:K], want[1]) and torch.equal(aligned[2][:K], want[2])
    for name, shifts in variants.items():
        assert any(v % 4 for v in shifts.values())
        rc, n, *got, outs = _raw_compact(t, keep, shifts)
        assert rc == 0 and n == K, (name, _abi.load().msr_last_error(None))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1][:K], want[1]) and torch.equal(got[2][:K], want[2]), name
        assert all(torch.equal(g, al) for g, al in zip(got, aligned)), name
        assert all(o.guards_untouched(K) for o in outs), (name, "guard elements or elements past the kept count written")


@pytest.mark.parametrize("P", ic.COMPACT_EDGE_P)
def test_scalar_compact_tile_edges(P):
    assert ic.constants()["COMPACT_TILE"] == ic.COMPACT_TILE
    rng = np.random.default_rng(P)
    t = ic.table(rng, 3000, 900, P)
    assert int(t[0][-1]) == P
    for frac in (0.01, 0.3, 0.9):
        _check_scalar_compact(t, rng.random(3000) >= frac, COMPACT_VARIANTS)


def test_scalar_compact_keep_all_keep_none_and_byte_offsets_8_and_12():
    rng = np.random.default_rng(6)
    t = ic.table(rng, 7000, 1500, 5 * ic.COMPACT_TILE + 17)
    _check_scalar_compact(t, np.ones(7000, bool), COMPACT_VARIANTS)
    _check_scalar_compact(t, np.zeros(7000, bool), COMPACT_VARIANTS)
    _check_scalar_compact(t, rng.random(7000) >= 0.3, {f"all+{4 * k}": dict.fromkeys(COMPACT_ARRAYS, k) for k in (2, 3)} |
                          {"mixed": dict(post_doc=3, post_tf=1, out_doc=2, out_tf=3)})


def test_scalar_compact_head_term_and_one_posting_terms():
    rng = np.random.default_rng(5)
    n = 60_000
    t = ic.table(rng, n, 3000, 30_000, head=n)               # term 0 spans ~29 tiles
    keep = rng.random(n) >= 0.01
    keep[1000:9000] = False
    _check_scalar_compact(t, keep, COMPACT_VARIANTS)
    many = ic.table(rng, 200_000, 100_000, 100_000)          # ~10^5 one-posting terms
    _check_scalar_compact(many, rng.random(200_000) >= 0.2, COMPACT_VARIANTS)
    tail = ic.table(rng, 5000, 4000, 40_000, empty_tail=700)
    _check_scalar_compact(tail, rng.random(5000) >= 0.5, COMPACT_VARIANTS)


def test_scalar_compact_refusals_leave_misaligned_outputs_untouched():
    rng = np.random.default_rng(3)
    t = ic.table(rng, 20_000, 800, 90_000)
    keep = rng.random(20_000) >= 0.1
    K = int(keep[t[1]].sum())
    shifts = COMPACT_VARIANTS["all"]

    def untouched(r):
        return bool((r[2] == GUARD).all()) and all(o.guards_untouched(0) for o in r[5])
    bad_off = t[0].copy()
    bad_off[100] = bad_off[101] + 1                          # not monotone
    r = _raw_compact((bad_off, t[1], t[2]), keep, shifts, K)
    assert r[0] == -1 and untouched(r)
    for bad in (20_000, -3):                                 # outside [0, n_docs)
        bad_doc = t[1].copy()
        bad_doc[77_777] = bad
        r = _raw_compact((t[0], bad_doc, t[2]), keep, shifts, K)
        assert r[0] == -1 and untouched(r)
    r = _raw_compact(t, keep, shifts, K - 1)                 # capacity below the count
    assert r[0] == -1 and r[1] == K and untouched(r)
    r = _raw_compact(t, keep, shifts, 0)                     # the sizing call writes nothing
    assert r[0] == 0 and r[1] == K and untouched(r)
    r = _raw_compact(t, keep, shifts, K)                     # and the well-formed call succeeds
    want = compact_postings(*t, keep)
    assert r[0] == 0 and r[1] == K and torch.equal(r[2], want[0]) and torch.equal(r[3], want[1]) and torch.equal(r[4], want[2])
    assert all(o.guards_untouched(K) for o in r[5])
