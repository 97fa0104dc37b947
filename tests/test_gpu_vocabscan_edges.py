"""The two vocabulary lookups (msr_fuzzy_terms, msr_wildcard_terms; csrc/msr_vocabscan.h, DESIGN K15, K16) where their first
tests do not go: an edit at every position of terms up to 32 code points over a wide alphabet with a signature collision, heads
and tails of every length and the general matcher on long runs, and a vocabulary of 258 spans whose rows take the merge kernel
through several rounds, skipped rounds, full 2048-key sorts and the second trip of its counting loop.  Raw ABI calls into
pre-filled buffers (the harnesses of test_gpu_fuzzy.py and test_gpu_wildcard.py), every output compared exactly with the
full-table oracles of vocabscan_cases.py, whose cases test_vocabscan_cases.py vouches for; and DeviceEngine's two calls on
lists of more than 1024 entries.  One engine per vocabulary and module; the expected rows are computed once."""
import numpy as np
import pytest
import torch

from msretr import _abi
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from test_gpu_fuzzy import Bound as FuzzyBound
from test_gpu_wildcard import Bound as WildBound
from vocabscan_cases import (COLLIDE, cut, edit_families, fuzzy_candidates, many_spans, pack, wild_candidates,
                             wild_long_cases)

pytestmark = pytest.mark.gpu
MAX_CALL = _abi.MSR_WILD_MAX_PATTERNS


def _bound(vocab, weights):
    """(fuzzy harness, wildcard harness) over ONE engine with the vocabulary bound."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    fz = FuzzyBound(vocab, weights)
    assert fz.rc == 0
    wc = WildBound.__new__(WildBound)
    wc.vocab, wc.weights, wc.eng, wc.rc = fz.vocab, fz.weights, fz.eng, 0
    return fz, wc


@pytest.fixture(scope="module")
def families():
    c = edit_families()
    c["cands"] = fuzzy_candidates(c["vocab"], c["weights"], c["words"], c["maxes"])
    fz, wc = _bound(c["vocab"], c["weights"])
    yield c, fz
    fz.close()


@pytest.fixture(scope="module")
def wild_long():
    c = wild_long_cases()
    c["cands"] = wild_candidates(c["vocab"], c["weights"], c["patterns"])
    fz, wc = _bound(c["vocab"], c["weights"])
    yield c, wc
    fz.close()


@pytest.fixture(scope="module")
def spans():
    c = many_spans()
    packed = pack(c["vocab"])
    c["fz"] = fuzzy_candidates(c["vocab"], c["weights"], c["words"], c["maxes"], packed)
    c["wc"] = wild_candidates(c["vocab"], c["weights"], c["patterns"], packed)
    fz, wc = _bound(c["vocab"], c["weights"])
    yield c, fz, wc
    fz.close()


# ------------------------------------------------------------------------------------------------ fuzzy: edit families
@pytest.mark.parametrize("limit", [1, 3, 16])
def test_an_edit_at_every_position_of_every_base_length(families, limit):
    c, b = families
    words, maxes = c["words"], c["maxes"]
    assert _abi.MSR_FUZZY_WORD_GROUP < len(words) <= _abi.MSR_FUZZY_MAX_WORDS and len(words) % _abi.MSR_FUZZY_WORD_GROUP == 0
    b.check(words, maxes, limit, want=cut(c["cands"], limit, True))
    # the same words the other way round: slot s of the LDS word group becomes slot 15 - s
    b.check(words[::-1], maxes[::-1], limit, want=cut(c["cands"][::-1], limit, True))


# ------------------------------------------------------------------------------------------------ wildcard: long cases
@pytest.mark.parametrize("limit", [1, 8, 16])
def test_heads_tails_and_the_matcher_on_long_terms(wild_long, limit):
    c, b = wild_long
    patterns = c["patterns"]
    assert len(patterns) > 3 * MAX_CALL
    for a in range(0, len(patterns), MAX_CALL):
        b.check(patterns[a:a + MAX_CALL], limit, want=cut(c["cands"][a:a + MAX_CALL], limit, False))


# ------------------------------------------------------------------------------------------------ both: many spans
@pytest.mark.parametrize("limit", [1, 3, 8, 16])
def test_fuzzy_rows_of_every_kind_over_258_spans(spans, limit):
    c, b, _ = spans
    assert b.eng.lib.msr_fuzzy_scratch_bytes(len(c["vocab"]), 1, 1) == 258 * (8 + 4)          # 258 spans
    want = cut(c["fz"], limit, True)
    first, _ = b.check(c["words"], c["maxes"], limit, want=want)
    if limit == 16:
        again = b.run(c["words"], c["maxes"], limit)
        assert b"".join(x.tobytes() for x in again) == b"".join(x.tobytes() for x in first)


@pytest.mark.parametrize("limit", [1, 3, 8, 16])
def test_wildcard_rows_of_every_kind_over_258_spans(spans, limit):
    c, _, b = spans
    want = cut(c["wc"], limit, False)
    first, _ = b.check(c["patterns"], limit, want=want)
    if limit == 16:
        again = b.run(c["patterns"], limit)
        assert b"".join(x.tobytes() for x in again) == b"".join(x.tobytes() for x in first)


# ------------------------------------------------------------------------------------------------ the engine's slices
def _named(vocab, weights):
    """-> (CorpusIndex whose vocabulary names each string once, by its first id, with the weights as document frequencies;
    the strings and weights the engine then serves: an id without a name has the empty string and weight 0)."""
    names = {}
    for t, s in enumerate(vocab):
        if s and s not in names:
            names[s] = t
    served = [s if names.get(s) == t else "" for t, s in enumerate(vocab)]
    served_w = [w if s and len(s) <= 32 else 0 for s, w in zip(served, weights)]
    df = np.asarray(weights, np.int64)
    n_docs = int(df.max()) + 1
    term_off = np.concatenate([[0], np.cumsum(df)]).astype(np.int64)
    post_doc = np.concatenate([np.arange(w, dtype=np.int32) for w in weights])
    ix = CorpusIndex(doc_ids=np.arange(n_docs, dtype=np.int64), doc_len=np.bincount(post_doc, minlength=n_docs).astype(np.int32) + 1,
                     term_off=term_off, post_doc=post_doc, post_tf=np.ones(len(post_doc), np.int32),
                     idf=np.ones(len(vocab), np.float32), avgdl=float(len(post_doc)) / n_docs + 1, total_docs=n_docs, vocab=names)
    return ix, served, served_w


@pytest.fixture(scope="module")
def named_engine():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    c = edit_families()
    ix, served, served_w = _named(c["vocab"], c["weights"])
    eng = DeviceEngine(ix, max_queries=4, max_k=16, rerank_max_docs=0)
    assert eng.has_vocab
    yield c, eng, served, served_w
    eng.close()


UNLOOKABLE = ["", "a" * 33, "ab\U0001F600", "x\uffff"]


def _scattered(some, n):
    """n entries drawn from `some` in an order that does not repeat with the slice length, an unlookable one every 41 entries
    -> (list, the positions of the lookable ones)."""
    out, ask = [], []
    while len(ask) < n:
        if len(out) % 41 == 17:
            out.append(UNLOOKABLE[len(out) // 41 % len(UNLOOKABLE)])
        else:
            i = len(ask)
            out.append(some[(7 * i + i // 50) % len(some)])
            ask.append(len(out) - 1)
    return out, ask


def test_engine_fuzzy_terms_slices_a_list_above_1024_words(named_engine):
    c, eng, served, served_w = named_engine
    bases = c["bases"]
    some = [(b, m) for b in (bases[3], bases[9], bases[15], bases[22]) for m in (0, 1, 2)]
    some += [(b[:-1] + COLLIDE[1], 2) for b in (bases[8], bases[19], bases[29])] + [(bases[2], 1), ("zzzz", 2)]
    assert len(some) == 17
    entries, ask = _scattered(some, _abi.MSR_FUZZY_MAX_WORDS + 37)
    assert len(ask) == 1061 and len(entries) > len(ask) + 20
    words = [e if isinstance(e, str) else e[0] for e in entries]
    maxes = [0 if isinstance(e, str) else e[1] for e in entries]
    cands = dict(zip(some, fuzzy_candidates(served, served_w, [w for w, _ in some], [m for _, m in some])))
    assert sum(len(x) > 3 for x in cands.values()) >= 8 and sum(len(x) == 0 for x in cands.values()) >= 1
    got = eng.fuzzy_terms(words, max_edits=maxes, limit=3)
    assert len(got) == len(entries)
    for i, e in enumerate(entries):
        if isinstance(e, str):
            assert got[i] == ([], 0), i
        else:
            x = cands[e]
            assert got[i] == ([(int(t), int(d)) for d, _, t in x[:3]], len(x)), (i, e)


def test_engine_wildcard_terms_slices_a_list_above_1024_patterns(named_engine):
    c, eng, served, served_w = named_engine
    bases = c["bases"]
    some = [bases[28][:3] + "*", "*" + bases[29][-3:], bases[27][:9] + "*" + bases[27][-8:], bases[26][:30] + "?*",
            "?" + bases[9][1:], bases[20], "*" + COLLIDE[1] + "*", "?", "??*", "*" + bases[5][4:8] + "*", "zz*", "*"]
    entries, ask = _scattered(some, _abi.MSR_WILD_MAX_PATTERNS + 37)
    assert len(ask) == 1061
    cands = dict(zip(some, wild_candidates(served, served_w, some)))
    assert sum(len(x) > 8 for x in cands.values()) >= 4 and sum(len(x) == 0 for x in cands.values()) >= 1
    got = eng.wildcard_terms(entries, limit=8)
    assert len(got) == len(entries)
    ask = set(ask)
    for i, e in enumerate(entries):
        if i in ask:
            x = cands[e]
            assert got[i] == ([int(t) for _, t in x[:8]], len(x)), (i, e)
        else:
            assert got[i] == ([], 0), i
