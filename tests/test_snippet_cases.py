"""Query-biased snippets, the CPU side (DESIGN K14): the oracle of snippet_ref.py against its two other formulations on every
case and on random draws; text.simple_tokenize_spans against simple_tokenize; snippets.term_weights / query_row / render; the
ABI constants of _abi.py against the header."""
import inspect
import os
import re

import numpy as np
import pytest

from msretr import _abi
from msretr.index import CorpusIndex
from msretr.index_build import normalise_document_text
from msretr.snippets import display_text, query_row, render, term_weights
from msretr.text import simple_tokenize, simple_tokenize_spans
from snippet_ref import (NONE, VARIANTS, best_window, best_window_2, best_windows_fast, corpus_cases, expected, hand, random_draws,
                         valid)

KEYS = ["hand"] + list(VARIANTS)


def _corpus(key):
    return hand() if key == "hand" else corpus_cases(*key)


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_the_three_formulations_agree_on_every_case(key):
    c, want = _corpus(key), expected(key)
    assert len(want) == len(c.pairs) > 0
    for (d, r, claim), w in zip(c.pairs, want):
        assert best_window_2(c.streams[d], c.rows[r], c.weights[r], c.spans[r]) == w, claim
    fast = best_windows_fast(c.tok_off, c.tok_ids, [p[0] for p in c.pairs], [p[1] for p in c.pairs], c.rows, c.weights, c.spans)
    assert [x.dtype for x in fast] == [np.int32, np.int32, np.int32, np.uint64, np.uint32]
    for i, w in enumerate(want):
        assert tuple(int(x[i]) for x in fast) == w, c.pairs[i]
    # pairs out of range, in the middle of valid ones
    docs, rows = [c.pairs[0][0], -1, c.n_docs, c.pairs[0][0], c.pairs[0][0]], [c.pairs[0][1]] * 3 + [-1, len(c.rows)]
    fast = best_windows_fast(c.tok_off, c.tok_ids, docs, rows, c.rows, c.weights, c.spans)
    assert [tuple(int(x[i]) for x in fast) for i in range(5)] == [want[0]] + [NONE] * 4


def test_the_hand_made_cases_say_what_they_claim():
    c, want = hand(), expected("hand")
    name = c.name
    one = lambda doc, row, weights, span: best_window(c.streams[name[doc]], row, weights, span)
    from phrase_ref import A, B, C_, L16
    W = _abi.MSR_SNIPPET_MAX_WEIGHT
    assert one("tie_0_2", [A, B], [3, 5], 4) == (3, 8, 2, 0b1100, 3)                   # not the equal window at 138
    assert one("best_2", [A, B, C_], [3, 5, 2], 4) == (139, 10, 3, 0b1110, 7)
    assert one("hits_2", [A, B], [3, 5], 4) == (139, 8, 3, 0b1110, 3)                  # the same cover, one hit more
    assert one("tie_end", [A], [9], 5) == (6, 9, 1, 1 << 4, 1)
    assert one("tie_end", [A], [9], 64) == (6, 9, 2, (1 << 4) | (1 << 63), 1)          # bit 63 of the mask
    assert one("short_best", [A, B], [3, 5], 64) == (0, 8, 2, 0b10100, 3)              # five tokens: bits 5 .. 63 are 0
    assert one("end_better", [A, B], [3, 5], 2) == (68, 8, 2, 0b11, 3)
    assert one("before_terms", [A, B, C_], [3, 5, 2], 64) == (0, 3, 1, 0b100, 1)       # B C of the next document are not seen
    assert one("third_chunk", [A], [9], 64) == (87, 9, 1, 1 << 63, 1)
    assert one("last_chunk", [A], [9], 5) == (295, 9, 1, 1 << 4, 1)
    assert one("l16", L16[::-1], [W] * 16, 16) == (3, 1 << 24, 16, 0xFFFF, 0xFFFF)
    assert one("repeat", [A, B, A], [3, 5, 1000], 64) == (0, 8, 4, 0b1000011010, 0b011)
    assert one("zero", [A, B], [0, 0], 3) == (3, 0, 2, 0b110, 0b11)                    # all weights 0: hits decide
    assert one("zero", [A, B], [W + 1, 5], 3) == NONE and one("zero", [A, B], [-1, 5], 3) == NONE
    assert one("zero", [A, B], [1, 1], 0) == NONE and one("zero", [A, B], [1, 1], 65) == NONE
    assert one("zero", [], [], 5) == NONE and one("l17", list(range(62, 79)), [1] * 17, 64) == NONE
    assert one("empty_between", [A], [1], 5) == NONE and one("zero", [C_], [1], 5) == NONE
    n_hit = sum(w != NONE for w in want)
    assert 150 < n_hit < len(want) - 50                      # the mix holds both kinds


def test_2000_random_draws():
    draws = random_draws(2000)
    n_none = n_valid = 0
    for s, p, w, span in draws:
        want = best_window(s, p, w, span)
        assert best_window_2(s, p, w, span) == want, (s, p, w, span)
        off, tok = np.array([0, len(s)], np.int64), np.asarray(s, np.int32)
        fast = best_windows_fast(off, tok, [0], [0], [p], [w], [span])
        assert tuple(int(x[0]) for x in fast) == want, (s, p, w, span)
        n_none += want == NONE
        n_valid += valid(p, w, span)
        if want != NONE:                                     # what every answer must satisfy, whatever found it
            a, cover, hits, mask, bits = want
            win = s[a:a + span]
            assert 0 <= a < len(s) and hits == bin(mask).count("1") >= 1 and mask >> len(win) == 0
            assert all((t in p) == bool(mask >> k & 1) for k, t in enumerate(win))
            assert cover == sum(w[j] for j in range(len(p)) if bits >> j & 1)
            assert all((bits >> j & 1) == (p[j] in win and p[j] not in p[:j]) for j in range(len(p)))
    assert 200 < n_none < 1200 and 1700 < n_valid < 1800


# ------------------------------------------------------------------------------------------------ the tokenizer with spans
TEXTS = ["Max Planck Institut in Tuebingen", "", "  ", "das 3 Planck-Institut, 2te Straße_x Äpfel ÖL", "İstanbul ǅ ß ſ x",
         "naïve café — Ελληνικά and русский 中文 text", "a1b2c3 __init__ x_y", "Tübingen\nTuebingen\tTUBINGEN"]


@pytest.mark.parametrize("text", TEXTS)
def test_simple_tokenize_spans_is_simple_tokenize_with_places(text):
    gen = simple_tokenize_spans(text)
    assert inspect.isgenerator(gen)                          # lazy: the renderer stops at its window's end
    got = list(gen)
    assert [t for t, _, _ in got] == simple_tokenize(text)
    assert all(text[b:e].lower() == t and b < e for t, b, e in got)
    assert all(got[i][2] <= got[i + 1][1] for i in range(len(got) - 1))


def test_simple_tokenize_spans_stops_where_the_caller_stops():
    seen = []
    gen = simple_tokenize_spans("alpha beta " * 100000)
    for item in gen:
        seen.append(item)
        if len(seen) == 3:
            break
    assert seen == [("alpha", 0, 5), ("beta", 6, 10), ("alpha", 11, 16)]
    assert next(gen) == ("beta", 17, 21)                     # the generator is still where the caller left it


# ------------------------------------------------------------------------------------------------ weights and rows
def _ix(idf):
    idf = np.asarray(idf, np.float32)
    return CorpusIndex(doc_ids=np.arange(1, dtype=np.int64), term_off=np.zeros(len(idf) + 1, np.int64), idf=idf)


def test_term_weights():
    ix = _ix([1.0, -0.3, 0.0, 0.0004, 0.00049, 2000.0, 1.5, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, 1023.99999])
    W = _abi.MSR_SNIPPET_MAX_WEIGHT
    # a negative idf (the appended city) and a zero one get the minimum; the cap; round-half-even of Python's round
    assert term_weights(ix, [0, 1, 2, 3, 4, 5, 6]) == [1024, 1, 1, 1, 1, W, 1536]
    assert term_weights(ix, [7, 8, 9]) == [1, 2, 2]
    assert term_weights(ix, [10]) == [W] and term_weights(ix, []) == []
    assert all(isinstance(w, int) for w in term_weights(ix, [0, 5]))
    for i, v in enumerate(np.asarray(ix.idf).tolist()):
        assert term_weights(ix, [i])[0] == max(1, min(1 << 20, round(1024 * max(v, 0))))


def test_query_row():
    idf = [0.1 * (1 + j % 7) for j in range(30)]
    idf[0] = -0.5                                            # the city
    ix = _ix(idf)
    assert query_row(ix, [5, 3, 5, -1, 30, 3, 0]) == [5, 3, 0]         # distinct, known, first-occurrence order
    assert query_row(ix, []) is None and query_row(ix, [-1, 30, 99]) is None
    assert query_row(ix, list(range(16))) == list(range(16))
    # more than 16: the 16 heaviest stay, of two equal ones the earlier, in first-occurrence order
    ids = list(range(20))
    w = term_weights(ix, ids)
    order = sorted(range(20), key=lambda j: (-w[j], j))[:16]
    got = query_row(ix, ids)
    assert got == sorted(order) and len(got) == 16 and 0 not in got
    assert w[1] == w[8] == w[15] and 1 in got and 8 in got and 15 not in got       # (the idf repeats with period 7)
    dropped = set(ids) - set(got)
    assert all(w[j] <= min(w[k] for k in got) for j in dropped)
    tie = [j for j in dropped if any(w[j] == w[k] for k in got)]
    assert tie and all(j > k for j in tie for k in got if w[k] == w[j])        # ties went to the earlier one
    ix2 = _ix([1.0] * 20)
    assert query_row(ix2, list(range(19, -1, -1))) == list(range(19, 3, -1))   # all equal: the first sixteen


# ------------------------------------------------------------------------------------------------ render
def _stream(title, text):
    return simple_tokenize(normalise_document_text(title, text))


def _check_render(title, text, start, mask, span, row_words, **kw):
    """The invariant: every highlighted slice, normalised and tokenised, is exactly one token, and it is a term of the row."""
    snippet, hl = render(title, text, start, mask, span, **kw)
    words = _stream(title, text)
    assert len(hl) == bin(mask).count("1")
    bits = [k for k in range(span) if mask >> k & 1]
    for k, (b, e) in zip(bits, hl):
        toks = simple_tokenize(normalise_document_text("", snippet[b:e]))
        assert toks == [words[start + k]] and toks[0] in row_words, (snippet, b, e)
    assert all(hl[i][1] <= hl[i + 1][0] for i in range(len(hl) - 1))
    return snippet, hl


def test_render_shows_the_raw_page_where_positions_hold():
    title, text = "Max Planck", "Das Institut für Biologie liegt in der Stadt, nahe der Universität."
    words = _stream(title, text)
    assert words[:4] == ["max", "planck", "das", "institut"]
    norm, shown = display_text(title, text)
    assert shown == f"{title} {text}" and norm == shown.lower()
    # a window in the middle: tokens 3 .. 5, highlights on 3 and 5
    s, hl = _check_render(title, text, 3, 0b101, 3, {"institut", "biologie"})
    assert s == "...Institut für Biologie..." and hl == [[3, 11], [16, 24]]
    # at the string's start: no dots in front; across the title / text seam (tokens 1 and 2)
    s, hl = _check_render(title, text, 0, 0b110, 3, {"planck", "das"})
    assert s == "Max Planck Das..." and hl == [[4, 10], [11, 14]]
    # at the string's end: the window is cut at the last token; the full stop behind it is the string's rest
    n = len(words)
    s, hl = _check_render(title, text, n - 2, 0b10, 64, {"universität"})
    assert s == "...der Universität..." and hl == [[7, 18]]
    s, hl = _check_render(title, "ende der Universität", 4, 0b1, 5, {"universität"})
    assert s == "...Universität" and hl == [[3, 14]]           # ends the string: no dots behind
    s, hl = _check_render("", "Wort", 0, 1, 30, {"wort"})
    assert s == "...Wort" and hl == [[3, 7]]                   # (title "" + " " + text: the seam's blank stands in front)
    # context_chars: widened to whole words, never past the string
    s, hl = _check_render(title, text, 3, 0b101, 3, {"institut", "biologie"}, context_chars=6)
    assert s == "...Das Institut für Biologie liegt..." and hl == [[7, 15], [20, 28]]
    s, hl = _check_render(title, text, 3, 0b1, 1, {"institut"}, context_chars=1000)
    assert s == f"{title} {text}" and hl == [[15, 23]]


def test_render_falls_back_to_the_normalised_string():
    # a city spelling: the normalisation changes the length, so the raw string's positions do not hold
    title, text = "Uni TUEBINGEN", "Die Mensa in Tuebingen hat Öffnungszeiten"
    norm, shown = display_text(title, text)
    assert shown == norm == "uni tübingen die mensa in tübingen hat öffnungszeiten"
    s, hl = _check_render(title, text, 3, 0b101, 3, {"mensa", "tübingen"})
    assert s == "...mensa in tübingen..." and hl == [[3, 8], [12, 20]]
    assert display_text("x", "Stadt Tubingen")[1] == "x stadt tübingen"
    # a character whose lower-casing is longer (U+0130 -> 'i' + U+0307): positions behind it move
    title, text = "İstanbul", "Reise nach İstanbul und Ankara"
    norm, shown = display_text(title, text)
    assert len(norm) > len(f"{title} {text}") and shown == norm
    words = _stream(title, text)
    k = words.index("ankara")
    s, hl = _check_render(title, text, k, 1, 1, {"ankara"})
    assert s == "...ankara" and hl == [[3, 9]]
    # the same page without the offending character is shown raw
    assert display_text("Istanbul", "Reise nach ANKARA")[1] == "Istanbul Reise nach ANKARA"
    # None title / text
    assert display_text(None, None) == (" ", " ") and display_text(None, "Ab")[1] == " Ab"


def test_render_refuses_what_does_not_fit_the_page():
    with pytest.raises(ValueError, match="no token"):
        render("", "eins zwei", 2, 1, 5)
    with pytest.raises(ValueError, match="past the page"):
        render("", "eins zwei", 1, 0b10, 5)
    for start, mask, span in ((-1, 1, 5), (0, 1, 0), (0, 1, 65), (0, 0b100, 2), (0, -1, 5)):
        with pytest.raises(ValueError):
            render("", "eins zwei", start, mask, span)


def test_render_with_a_custom_span_tokenizer_and_on_random_windows():
    # a tokenizer that drops stop words: token positions skip them, the spans still point into the page
    stop = {"der", "die", "das", "in", "für"}
    spans_fn = lambda text: ((t, b, e) for t, b, e in simple_tokenize_spans(text) if t not in stop)
    title, text = "Das Haus", "Die Mensa in der Stadt für alle"
    s, hl = render(title, text, 1, 0b11, 2, spans_fn)        # tokens: haus mensa stadt alle
    assert s == "...Mensa in der Stadt..." and hl == [[3, 8], [16, 21]]
    rng = np.random.default_rng(4)
    vocab = ["Alpha", "beta", "GAMMA", "Straße", "Äpfel", "x"]
    for i in range(200):
        words = [vocab[j] for j in rng.integers(0, len(vocab), int(rng.integers(1, 40)))]
        cut = int(rng.integers(0, len(words) + 1))
        title, text = " ".join(words[:cut]), ", ".join(words[cut:])
        stream = _stream(title, text)
        assert len(stream) == len(words)
        span = int(rng.integers(1, 65))
        start = int(rng.integers(0, len(stream)))
        n = min(span, len(stream) - start)
        mask = int(rng.integers(0, 1 << min(n, 62)))
        _check_render(title, text, start, mask, span, {w.lower() for w in vocab}, context_chars=int(rng.integers(0, 3)) * 7)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_and_header_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msretr.h"), encoding="utf-8").read()
    assert int(re.search(r"#define MSR_ABI_VERSION (\d+)", hdr).group(1)) == _abi.MSR_ABI_VERSION == 16
    m = re.search(r"#define MSR_SNIPPET_MAX_WEIGHT \(1 << (\d+)\)", hdr)
    assert m and 1 << int(m.group(1)) == _abi.MSR_SNIPPET_MAX_WEIGHT == 1 << 20
    assert _abi.MSR_PHRASE_MAX_TERMS * _abi.MSR_SNIPPET_MAX_WEIGHT == 1 << 24     # the largest cover, exact in an int32
    assert "msr_best_windows" in hdr and "msr_best_windows" in _abi._SIGNATURES
    assert len(_abi._SIGNATURES["msr_best_windows"][1]) == 15
