"""Rows beyond one launch: msr_term_sets, msr_phrase_sets, msr_proximity_sets and msr_combine_sets cut a call into launches of at
most 32 768 rows (the grid's y extent) and tell each launch its first row.  No other test asks for that many rows, and a wrong
first row is invisible below the cut.  32 770 rows cycle through 7 row definitions (7 is odd: the cycle does not line up with
the cut) over the 70-document corpus of phrase_ref.py -- one span, 3 words per row, a 6-bit tail -- so the oracle runs 7
times per entry point; every output row is compared word for word, the word behind each row keeps its fill, and a second call
gives the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr.docset import pack_bits
from msretr.engine import DeviceEngine
from phrase_ref import A, B, C_, D, E, F, UNUSED, X, Y, cand_mask, combine_mask, corpus, phrase_mask_fast
from proximity_ref import near_mask_fast

pytestmark = pytest.mark.gpu
N = 70
R = 32770                                                    # two launches: rows 0 .. 32767 and 32768 .. 32769
M = 7
FILL = 0xA5A5A5A5


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a if len(a) else [0], np.int32)).to(dev)


def _csr(lists, dev):
    """lists[i % M] for i < R as (offsets [R + 1], values) on the device."""
    off, flat = [0], []
    for i in range(R):
        flat += lists[i % M]
        off.append(len(flat))
    return _i32(off, dev), _i32(flat, dev)


def _col(values, dev):
    return _i32([values[i % M] for i in range(R)], dev)


@pytest.fixture(scope="module")
def setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    c = corpus(N)
    eng = DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0)
    assert eng.has_tokens
    W = (N + 31) // 32
    rows = np.full((len(c.cands), W + 2), 0xFFFFFFFF, np.uint32)     # padding words and the bits at or above N are set
    for i, (_, m) in enumerate(c.cands):
        rows[i, :W] = pack_bits(m)
        rows[i, W - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    yield c, eng, torch.from_numpy(rows.view(np.int32)).to(eng.device), W + 2
    eng.close()


def _term_docs(c, t):
    """bool [N]: the documents whose stream holds term t (the index was built from the streams)."""
    out = np.zeros(N, bool)
    if 0 <= t < c.ix.n_terms:
        out[np.repeat(np.arange(N), np.diff(c.tok_off))[c.tok_ids == t]] = True
    return out


def _every(m):
    return np.ones(N, bool) if m is None else m


def _term_sets(c, eng, sets, stride, out, os_):
    odd, rnd, nc = c.cand("odd"), c.cand("rnd"), len(c.cands)
    #       must          must not    base
    defs = [([A],         [],         -1),                   # matches
            ([A, UNUSED], [],         -1),                   # valid, matches nothing: a term without a posting
            ([-1],        [],         -1),                   # invalid: an id out of range
            ([],          [F],        -1),
            ([B],         [C_],       odd),                  # names a base row
            ([],          [],         rnd),
            ([3],         [5, 99],    nc)]                   # a base row out of range: empty
    want = []
    for must, nots, base in defs:
        m = _every(cand_mask(c, base)).copy()
        for t in must:
            m &= _term_docs(c, t)
        for t in nots:
            m &= ~_term_docs(c, t)
        want.append(m)
    dev = eng.device
    m_off, m_ = _csr([d[0] for d in defs], dev)
    x_off, x_ = _csr([d[1] for d in defs], dev)
    rb = _col([d[2] for d in defs], dev)
    call = lambda: eng.lib.msr_term_sets(eng.handle, R, _P(m_off), _P(m_), _P(x_off), _P(x_), _P(sets), len(c.cands), stride, _P(rb),
                                         _P(out), os_, eng._stream())
    return want, call


def _phrase_sets(c, eng, sets, stride, out, os_):
    odd, rnd, nc = c.cand("odd"), c.cand("rnd"), len(c.cands)
    defs = [([A, B], -1),                                    # matches
            ([X, Y], -1),                                    # valid, matches nothing: only across document boundaries
            ([], -1),                                        # invalid: empty
            ([A, -1], -1),                                   # invalid: an id out of range
            ([A, B], odd),                                   # names a candidate row
            ([C_, D], rnd),
            ([A, B], nc)]                                    # a candidate row out of range: empty
    want = [phrase_mask_fast(c.tok_off, c.tok_ids, p, cand_mask(c, r)) for p, r in defs]
    dev = eng.device
    off, terms = _csr([d[0] for d in defs], dev)
    rc = _col([d[1] for d in defs], dev)
    call = lambda: eng.lib.msr_phrase_sets(eng.handle, R, _P(off), _P(terms), _P(sets), len(c.cands), stride, _P(rc), _P(out), os_,
                                           eng._stream())
    return want, call


def _proximity_sets(c, eng, sets, stride, out, os_):
    odd, rnd = c.cand("odd"), c.cand("rnd")
    #       terms     span ordered row_cand
    defs = [([B, A],  2,   0,      -1),                      # matches (A B stands in several documents)
            ([X, Y],  4,   1,      -1),                      # valid, matches nothing: X never stands in front of Y in a document
            ([],      5,   0,      -1),                      # invalid: empty
            ([A, B],  65,  0,      -1),                      # invalid: the span
            ([A, B],  2,   1,      odd),                     # names a candidate row
            ([C_, E], 3,   1,      rnd),
            ([A, C_], 64,  0,      -1)]
    want = [near_mask_fast(c.tok_off, c.tok_ids, p, s, bool(o), cand_mask(c, r)) for p, s, o, r in defs]
    dev = eng.device
    off, terms = _csr([d[0] for d in defs], dev)
    span, order, rc = (_col([d[k] for d in defs], dev) for k in (1, 2, 3))
    call = lambda: eng.lib.msr_proximity_sets(eng.handle, R, _P(off), _P(terms), _P(span), _P(order), _P(sets), len(c.cands), stride,
                                              _P(rc), _P(out), os_, eng._stream())
    return want, call


def _combine_sets(c, eng, sets, stride, out, os_):
    odd, edges, rnd, none = (c.cand(n) for n in ("odd", "edges", "rnd", "none"))
    #       AND            NOT
    defs = [([odd],        []),                              # matches
            ([odd, none],  []),                              # valid, matches nothing
            ([-1],         []),                              # invalid: a row out of range empties the AND
            ([],           [edges]),
            ([odd, rnd],   [edges]),
            ([],           []),
            ([rnd],        [999])]                           # a row out of range is ignored in the NOT
    masks = [m for _, m in c.cands]
    want = [combine_mask(masks, a, x, N) for a, x in defs]
    dev = eng.device
    a_off, a_ = _csr([d[0] for d in defs], dev)
    x_off, x_ = _csr([d[1] for d in defs], dev)
    call = lambda: eng.lib.msr_combine_sets(eng.handle, R, _P(a_off), _P(a_), _P(x_off), _P(x_), _P(sets), len(c.cands), stride,
                                            _P(out), os_, eng._stream())
    return want, call


@pytest.mark.parametrize("entry", [_term_sets, _phrase_sets, _proximity_sets, _combine_sets], ids=lambda f: "msr" + f.__name__)
def test_rows_beyond_one_launch(setup, entry):
    c, eng, sets, stride = setup
    dev, W = eng.device, (N + 31) // 32
    out = torch.from_numpy(np.full((R, W + 1), FILL, np.uint32).view(np.int32)).to(dev)
    want, call = entry(c, eng, sets, stride, out, W + 1)
    assert want[0].any() and not want[1].any() and not want[2].any(), "definitions 0 / 1 / 2: matching, non-matching, invalid"
    assert len({w.tobytes() for w in want}) >= 4             # a row written for another definition would show
    assert call() == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy().view(np.uint32)
    words = np.stack([pack_bits(w) for w in want])[np.arange(R) % M]
    for i in (32767, 32768, 32769):
        assert (got[i, :W] == words[i]).all(), f"row {i} (definition {i % M}): {got[i, :W]} != {words[i]}"
    wrong = np.nonzero((got[:, :W] != words).any(axis=1))[0]
    assert wrong.size == 0, f"{wrong.size} rows differ from their definition's, the first ones {wrong[:8].tolist()}"
    assert (got[:, W] == FILL).all(), "the word behind a row was touched"
    out.copy_(torch.from_numpy(np.full((R, W + 1), FILL, np.uint32).view(np.int32)))
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert out.cpu().numpy().tobytes() == got.tobytes()      # a second call: the same bytes
