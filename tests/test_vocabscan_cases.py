"""The vectorised oracles and the case generators of vocabscan_cases.py without a GPU (DESIGN K15, K16): osa_all and glob_all
against the plain loops of fuzzy_ref.py and wildcard_ref.py, and what the generators promise -- every edit at every position of
every base length, the signature collision and its m-bit edges, five lengths in one wave, heads and tails of every length on
both parities, and every kind of row the merge kernel can meet on 258 spans -- asserted on the oracle alone.  These conditions
are what gives test_gpu_vocabscan_edges.py its teeth."""
import numpy as np
import pytest

import fuzzy_ref
import wildcard_ref
from fuzzy_ref import MAX_LEN, osa
from vocabscan_cases import (ALPHABET, BASE_LENGTHS, BASE_LETTERS, COLLIDE, MG_CAP, N_SPANS_TERMS, NEW_LETTERS, ROW_WORDS,
                             SINGLE_KINDS, SPAN, WAVE, X_SPANS, cut, edit_families, fuzzy_candidates, glob_all, many_spans,
                             osa_all, pack, rounds_of, sig_bit, signature, wild_candidates, wild_long_cases)
from wildcard_ref import glob_match


@pytest.fixture(scope="module")
def families():
    c = edit_families()
    c["cands"] = fuzzy_candidates(c["vocab"], c["weights"], c["words"], c["maxes"])
    return c


@pytest.fixture(scope="module")
def wild_long():
    c = wild_long_cases()
    c["cands"] = wild_candidates(c["vocab"], c["weights"], c["patterns"])
    return c


@pytest.fixture(scope="module")
def spans():
    c = many_spans()
    packed = pack(c["vocab"])
    c["fz"] = fuzzy_candidates(c["vocab"], c["weights"], c["words"], c["maxes"], packed)
    c["wc"] = wild_candidates(c["vocab"], c["weights"], c["patterns"], packed)
    return c


def _popcount(v):
    return bin(v).count("1")


# ------------------------------------------------------------------------------------------------ the oracles
def test_osa_all_on_the_known_answers():
    for a, b, d in fuzzy_ref.KNOWN:
        assert osa_all(a, [b, a, ""]).tolist() == [d, 0, len(a)] and osa_all(b, [a]).tolist() == [d], (a, b)
    assert osa_all("", ["", "ab"]).tolist() == [0, 2]
    vocab, _, words = fuzzy_ref.hand()
    for w in words:
        assert osa_all(w, vocab).tolist() == [osa(w, s) for s in vocab], w


def test_glob_all_on_the_known_answers():
    for p, answers in wildcard_ref.KNOWN:
        assert glob_all(p, list(answers)).tolist() == list(answers.values()), p
    vocab, _, patterns = wildcard_ref.hand()
    for p in patterns:
        assert glob_all(p, vocab).tolist() == [glob_match(p, s) for s in vocab], p


def _sample(rng, rows, cands, vocab, k):
    """k (row, term) pairs: of 40 rows at random; the term a candidate of the row every other time, any term otherwise."""
    some = rng.choice(len(rows), min(40, len(rows)), replace=False)         # (one table per row: not too many of them)
    for i in range(k):
        r = int(some[int(rng.integers(0, len(some)))])
        if i % 2 and len(cands[r]):
            t = int(cands[r][int(rng.integers(0, len(cands[r]))), -1])
        else:
            t = int(rng.integers(0, len(vocab)))
        yield r, t


def test_osa_all_on_sampled_pairs_of_each_generator(families, spans):
    rng = np.random.default_rng(1)
    for c, cands in ((families, families["cands"]), (spans, spans["fz"])):
        packed = pack(c["vocab"])
        table, seen = {}, 0
        for r, t in _sample(rng, c["words"], cands, c["vocab"], 400):
            w = c["words"][r]
            if w not in table:
                table[w] = osa_all(w, packed)
            assert table[w][t] == osa(w, c["vocab"][t]), (w, c["vocab"][t])
            seen += table[w][t] <= 2
        assert seen >= 100                                   # near pairs among them, not only far ones


def test_glob_all_on_sampled_pairs_of_each_generator(wild_long, spans):
    rng = np.random.default_rng(2)
    for c, cands in ((wild_long, wild_long["cands"]), (spans, spans["wc"])):
        packed = pack(c["vocab"])
        table, hits = {}, 0
        for r, t in _sample(rng, c["patterns"], cands, c["vocab"], 400):
            p = c["patterns"][r]
            if p not in table:
                table[p] = glob_all(p, packed)
            assert table[p][t] == glob_match(p, c["vocab"][t]), (p, c["vocab"][t])
            hits += bool(table[p][t])
        assert 100 <= hits <= 300


def test_cut_gives_what_the_plain_expected_gives():
    vocab, weights, words = fuzzy_ref.hand()
    maxes = [(3 * i + 1) % 4 for i in range(len(words))]
    for limit in (1, 3, 16):
        got = cut(fuzzy_candidates(vocab, weights, words, maxes), limit, True)
        for g, w in zip(got, fuzzy_ref.expected(vocab, weights, words, maxes, limit)):
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all()
    vocab, weights, patterns = wildcard_ref.hand()
    for limit in (1, 8):
        got = cut(wild_candidates(vocab, weights, patterns), limit, False)
        for g, w in zip(got, wildcard_ref.expected(vocab, weights, patterns, limit)):
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all()


# ------------------------------------------------------------------------------------------------ the alphabet
def test_the_alphabet_and_its_collision():
    assert len(ALPHABET) == len(set(ALPHABET)) >= 30 and set("äöüß\ufffe") <= set(ALPHABET)
    assert sum(ord(c) >= 0x8000 for c in ALPHABET) >= 2 and max(map(ord, ALPHABET)) == 0xFFFE
    a, b = COLLIDE
    assert a != b and a in BASE_LETTERS and b in ALPHABET and b not in BASE_LETTERS + NEW_LETTERS
    assert sig_bit(ord(a)) == sig_bit(ord(b)) and signature(a) == signature(b)
    bits = [sig_bit(ord(c)) for c in BASE_LETTERS + NEW_LETTERS]
    assert len(set(bits)) == len(bits)                       # every other letter has a bit of its own: the edges below are exact
    assert sig_bit(0) == 0 and sig_bit(1) == 0x9E3779B1 >> 26 and sig_bit(0xFFFE) == ((0xFFFE * 0x9E3779B1) % 2 ** 32) >> 26


# ------------------------------------------------------------------------------------------------ fuzzy: edit families
def test_every_edit_at_every_position_is_found_at_its_distance(families):
    c = families
    vocab, weights, meta, words, maxes = c["vocab"], c["weights"], c["meta"], c["words"], c["maxes"]
    assert 3 <= -(-len(vocab) // SPAN) <= 6 and 3000 <= len(vocab)
    assert len(c["bases"]) == 3 * len(BASE_LENGTHS) and sorted({len(b) for b in c["bases"]}) == list(BASE_LENGTHS)
    want = set()
    for f, b in enumerate(c["bases"]):
        n = len(b)
        want |= {(f, n, k, p) for k in ("sub", "sub_collide", "del") for p in range(n)}
        want |= {(f, n, "ins", p) for p in range(n + 1)} | {(f, n, "swap", p) for p in range(n - 1)}
    assert want <= {m[:4] for m in meta} and {m[2] for m in meta} >= set(SINGLE_KINDS)
    found = {}                                               # family -> {term: distance} of the base at tolerance 2
    for w, m, cand in zip(words, maxes, c["cands"]):
        if m == 2 and w in c["bases"] and c["bases"].index(w) not in found:
            found[c["bases"].index(w)] = {int(t): int(d) for d, _, t in cand}
    assert len(found) == len(c["bases"])
    singles = doubles = triples = long_ones = 0
    for t, (f, n, kind, p, d) in enumerate(meta):
        if kind == "dead":
            assert weights[t] == 0 and t not in found[f]
        elif len(vocab[t]) > MAX_LEN:                        # 33 or 34 code points: live, never a candidate
            assert weights[t] > 0 and len(vocab[t]) in (33, 34) and t not in found[f]
            long_ones += 1
            singles += kind in SINGLE_KINDS                  # (the 33 insertions into a base of 32)
        elif d is not None and d <= 2:
            assert weights[t] > 0 and found[f].get(t) == d == osa(c["bases"][f], vocab[t]), (kind, n, p)
            singles += kind in SINGLE_KINDS
            doubles += d == 2
        elif d == 3:
            assert weights[t] > 0 and t not in found[f] and osa(c["bases"][f], vocab[t]) >= 3, (kind, n, p)
            triples += 1
    assert singles == len(want) and doubles >= 500 and triples >= 80 and long_ones >= 100
    # the length-32 words: an insertion made them out of 31; and a swap on either side of a register boundary
    assert any(len(w) == 32 and any(len(vocab[int(t)]) == 31 and d == 1 for d, _, t in cand)
               for w, cand in zip(words, c["cands"]))
    assert {p & 1 for _, n, k, p, _ in meta if k == "swap" and n >= 29} == {0, 1}
    assert {m[3] for m in meta if m[2] == "swap" and m[1] == 32} == set(range(31))
    # the weights: few values, many repeats, so a row's order rests on the distance, the weight and the id
    assert len(set(weights)) <= 6
    d_w = [(int(d), int(w)) for d, w, _ in c["cands"][words.index(c["bases"][-1]) + 2]]
    assert len(d_w) > len(set(d_w)) > len({d for d, _ in d_w}) == 3
    totals = np.asarray([len(x) for x in c["cands"]])
    assert (totals > 16).sum() >= 20 and (totals == 1).sum() >= 10 and ((totals > 1) & (totals <= 16)).sum() >= 10


def test_signature_differences_of_exactly_m_bits_and_of_none(families):
    c = families
    edge = {1: 0, 2: 0}
    merged = 0
    for w, m, cand in zip(c["words"], c["maxes"], c["cands"]):
        sw = signature(w)
        for d, _, t in cand:
            st = signature(c["vocab"][int(t)])
            if m and _popcount(sw & ~st) == m and _popcount(st & ~sw) == m:
                edge[m] += 1
            if d == 1 and st == sw and COLLIDE[1] in c["vocab"][int(t)] and len(w) == len(c["vocab"][int(t)]):
                merged += 1                                  # a substitution the signature cannot see: the colliding pair
    assert edge[1] >= 100 and edge[2] >= 100 and merged >= 10


def test_five_lengths_of_one_family_stand_in_one_wave(families):
    c = families
    for f, b in enumerate(c["bases"]):
        n = len(b)
        cand = c["cands"][c["words"].index(b) + 2]
        assert c["maxes"][c["words"].index(b) + 2] == 2
        per_wave = {}
        for _, _, t in cand:
            per_wave.setdefault(int(t) // WAVE, set()).add(len(c["vocab"][int(t)]))
        most = max(len(v) for v in per_wave.values())
        assert most == min(n + 2, MAX_LEN) - max(n - 2, 0) + 1, (n, most)
        if 2 <= n <= 30:
            assert most == 5


# ------------------------------------------------------------------------------------------------ wildcard: long cases
def test_wild_long_cases_cover_every_head_tail_and_slot(wild_long):
    c = wild_long
    vocab, patterns, kinds, cands = c["vocab"], c["patterns"], c["kinds"], c["cands"]
    assert {len(s) for s in vocab} >= set(range(1, 34)) and set("".join(vocab)) <= set(ALPHABET)
    assert [len(t) for t in c["longs"]] == [32, 31, 30] and "aab" * 10 in vocab
    matched = [set(int(t) for _, t in x) for x in cands]
    seen = set()
    for t in c["longs"]:
        L, tid = len(t), vocab.index(t)
        for i, (kind, Lk, h, tl) in enumerate(kinds):
            if Lk != L or kind == "plain":
                continue
            seen.add((L, kind, h, tl))
            p = patterns[i]
            if len(p) > MAX_LEN:
                assert not matched[i]                        # 33 symbols and more: an empty row
            elif h + tl <= L:
                assert tid in matched[i], p
            else:
                assert h + tl == L + 1 and tid not in matched[i], p
        assert {(L, "head", h, 0) for h in range(L + 1)} | {(L, "tail", 0, h) for h in range(L + 1)} <= seen
        assert {(L, k, h, 0) for k in ("head?",) for h in range(1, L + 1)} <= seen
        assert {(L, "both", h, s - h) for s in (L - 1, L, L + 1) for h in range(L + 1) if 0 <= s - h <= L} <= seen
        # one `?` in every slot of every head and of every tail
        for kind, star in (("head?", -1), ("tail?", 0)):
            slots = {(h + tl, p.index("?") - (star == 0)) for p, (k, Lk, h, tl) in zip(patterns, kinds) if k == kind and Lk == L}
            assert slots == {(n, s) for n in range(1, L + 1) for s in range(n)}
        # ... and through every slot of the combined patterns, on both sides of the star
        both = [(p, h) for p, (k, Lk, h, tl) in zip(patterns, kinds) if k == "both?" and Lk == L]
        assert {p.index("?") for p, h in both if p.index("?") < h} >= set(range(L - 2))
        assert {len(p) - 1 - p.index("?") for p, h in both if p.index("?") > h} >= set(range(L - 2))
    # head + tail == L exactly and L + 1 inside 32 symbols: the 31- and the 30-code-point term
    fits = {(Lk, h + tl - Lk) for p, (k, Lk, h, tl) in zip(patterns, kinds) if k == "both" and len(p) <= MAX_LEN}
    assert fits >= {(32, -1), (31, -1), (31, 0), (30, -1), (30, 0), (30, 1)}
    plain = [p for p, k in zip(patterns, kinds) if k[0] == "plain"]
    assert all(len(p) == 32 and "*" not in p for p in plain) and {p.index("?") for p in plain if p.count("?") == 1} == set(range(32))
    # the general patterns: on the long runs, matching and not, `?` inside segments and in heads and tails around a middle
    gen = [i for i, k in enumerate(kinds) if k[0] == "general"]
    assert {"*ab*ab*b", "a*?b*?c", "*a**b*"} <= {patterns[i] for i in gen} and len(gen) >= 200
    runs = {t for t, s in enumerate(vocab) if len(s) >= 30 and set(s) <= set("abc")}
    hit = [i for i in gen if matched[i] & runs]
    pairs = sum(len(matched[i] & runs) for i in gen)         # (pattern, long run) pairs: the matcher says yes, and says no
    assert len(hit) >= 100 and len(gen) - len(hit) >= 5 and pairs >= 500 and len(gen) * len(runs) - pairs >= 500
    assert sum("?" in patterns[i] and patterns[i][0] != "*" != patterns[i][-1] for i in hit) >= 20
    totals = np.asarray([len(x) for x in cands])
    assert (totals > 16).sum() >= 100 and (totals == 0).sum() >= 100 and (totals == 1).sum() >= 100


# ------------------------------------------------------------------------------------------------ both: many spans
def _round(span, limit):
    return span // ((MG_CAP - limit) // limit)


def test_the_merge_rounds_at_each_limit():
    n_spans = -(-N_SPANS_TERMS // SPAN)
    assert n_spans == 258 and N_SPANS_TERMS == 257 * 1024 + 1
    assert rounds_of(16, n_spans) == [(0, 127), (127, 254), (254, 258)]
    assert rounds_of(8, n_spans) == [(0, 255), (255, 258)]
    assert rounds_of(3, n_spans) == [(0, 258)] == rounds_of(1, n_spans)


@pytest.mark.parametrize("lookup", ["fz", "wc"])
def test_many_spans_hold_every_kind_of_row(spans, lookup):
    c = spans
    vocab, weights = c["vocab"], c["weights"]
    assert len(vocab) == N_SPANS_TERMS and min(weights) >= 1 and max(len(s) for s in vocab) <= 8
    assert max(len(w) for w in c["words"]) <= 10            # every span is fully live
    cands = c[lookup]
    row = {}
    for i, tag in enumerate(c["tags"][:len(ROW_WORDS)]):
        x = cands[i]
        # a candidate's key as the kernels order it, its span, its round at limit 16
        keys = [tuple(int(v) for v in (r[0], -r[1], r[2])) if lookup == "fz" else (-int(r[0]), int(r[1])) for r in x]
        assert keys == sorted(keys)
        row[tag] = (keys, [int(r[-1]) // SPAN for r in x], [_round(int(r[-1]) // SPAN, 16) for r in x])
    assert [set(row[k][2]) for k in ("first", "middle", "last")] == [{0}, {1}, {2}]
    assert all(0 < len(row[k][0]) <= 16 for k in ("first", "middle", "last"))
    keys, sp, rd = row["each"]
    assert len(keys) > 16 and set(rd[:16]) == {0, 1, 2}     # the best 16 come from all three rounds
    assert {_round(s, 8) for s in sp[:8]} == {0, 1}          # ... and from both rounds at limit 8
    for tag, later_better in (("better_later", True), ("worse_later", False)):
        keys, sp, rd = row[tag]
        by_round = [[k for k, r in zip(keys, rd) if r == q] for q in range(3)]
        assert len(by_round[0]) >= 16 and by_round[1] and by_round[2]
        if later_better:
            assert max(by_round[2]) < min(by_round[1]) and max(by_round[1]) < min(by_round[0])
        else:
            assert max(by_round[0]) < min(by_round[1]) and max(by_round[0]) < min(by_round[2])
    keys, sp, rd = row["dense"]
    per_span = np.bincount(sp, minlength=258)
    assert (per_span > 16).sum() >= 130 and (per_span[:127] > 16).all()      # a whole round of full lists: P = 2048
    assert per_span[256] > 16 and len(keys) > 2000
    assert row["one_257"][1] == [257] and row["one_256"][1] == [256] and row["none"][0] == []
    if lookup == "wc":
        pat = dict(zip(c["patterns"], cands))
        x_spans = np.bincount(pat["x*"][:, 1] // SPAN, minlength=258)
        whole = np.flatnonzero(x_spans == SPAN)
        assert 10000 <= len(pat["x*"]) < 100000 and len(whole) >= 8 and set(whole) <= set(X_SPANS)
        assert len(pat["*"]) == N_SPANS_TERMS                # the sum over 258 spans of 1024, through both trips of the stride loop
        assert 0 < len(pat["x*7"]) < len(pat["x*"]) and len(pat["??????"]) > 200000
        for tag, p in zip(c["tags"], c["patterns"]):
            if tag:
                assert p == ROW_WORDS[tag][:2] + "*"
    else:
        assert c["words"][:len(ROW_WORDS)] == list(ROW_WORDS.values()) and set(c["maxes"]) == {1, 2}
        assert {d for d, _, _ in row["dense"][0]} == {1, 2} and {k[0] for k in row["better_later"][0]} == {0, 1, 2}
