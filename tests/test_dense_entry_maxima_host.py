"""Tile maxima recovered from the emitted entries (msr_gemm_f32_pass), restated in numpy.

The 256-query emit pass over the f32 rows stores no tile maxima.  The three selects behind it -- the raise between the
segments (thr'), the bucket's bound (thr2) and the sharded bound (out_part) -- are each "the j-th largest tile maximum,
j <= k", read from a matrix that holds -inf except where an entry (row, query, score, tile) has been joined in by an atomic
maximum on the float's bits.  Checked here, per query, on random and adversarial tile layouts:

* the join on bits (signed maximum for a clear sign bit, unsigned minimum for a set one, -inf to start with) leaves the
  largest score of each tile, up to the sign of a zero, which msr_ord32 does not tell apart;
* over [0, T1): every j-th largest true maximum (j <= k) at or above the emission threshold is the j-th largest entry maximum;
  a j-th largest true maximum below it leaves an entry value below it too (or none); thr' follows, raised or not;
* over all tiles, for the segmented pass (thr, then thr') and the one-launch pass (thr throughout): the j-th largest entry
  maximum IS the j-th largest true maximum for every j <= k; thr2 and out_part follow.

Emission compares against the threshold rounded DOWN to f16, as the kernel does.  Values are compared as msr_ord32 keys
(-0.0 and 0.0 share one), thresholds as bits."""
import numpy as np

from test_dense_segments_host import ROWS, _down_f16

NINF = np.float32(-np.inf)


def _key(x):
    """msr_ord32: larger float <=> larger key; -0.0 and 0.0 share a key."""
    x = np.asarray(x, dtype=np.float32)
    u = np.where(x == 0, np.float32(0), x).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _join(n_tiles, tile, score, order):
    """gemm_entry_tmax_kernel: the entries in the given order, one atomic on the float's bits each."""
    m = np.full(n_tiles, NINF, dtype=np.float32)
    w = m.view(np.uint32)
    for i in order:
        b = _bits(score[i:i + 1])[0]
        t = tile[i]
        if b & np.uint32(0x80000000):
            w[t] = min(w[t], b)                                  # unsigned minimum
        else:
            w[t] = np.uint32(max(np.int32(w[t]), np.int32(b)))   # signed maximum
    return m


def _kth_valid(v, j):
    """gemm_kth_kernel's select: the j-th largest value > -inf, or None for a short row."""
    v = v[v > NINF]
    return None if len(v) < j else np.sort(v)[-j]


def _thr(v, k, margin, scale=np.float32(1.0)):
    x = _kth_valid(v, k)
    return None if x is None else np.float32(np.float32(x) - np.float32(scale * margin))


def _raise(thr, v, k, margin):
    x = _thr(v, k, margin)
    return thr if x is None or not x > thr else x


def _check(score, T, k, t1, margin, rng, stats):
    """score: [T * ROWS] filter scores of one query (-inf: a row behind a short tile); t1 = 0: one emit launch."""
    tile_of = np.arange(T * ROWS) // ROWS
    tmax = score.reshape(T, ROWS).max(axis=1)
    ss = min(64, max(1, T // (3 * k)))
    thr = _thr(tmax[ss // 2::ss], k, margin)                     # the sample pass stores its maxima: true ones
    assert thr is not None
    e1 = _down_f16(thr)

    def entry_maxima(ethr):
        """ethr: [T] the emission threshold of each tile's launch (+inf: not visited yet)."""
        idx = np.flatnonzero(score >= ethr[tile_of])
        m = _join(T, tile_of, score, rng.permutation(idx))
        assert np.array_equal(_key(m[m > NINF]), _key(tmax[m > NINF]))     # a tile with entries holds its true maximum
        assert np.all(tmax[m == NINF] < ethr[m == NINF])                   # ... one without is below its threshold
        return m

    if t1:
        seg1 = np.arange(T) < t1
        m1 = entry_maxima(np.where(seg1, e1, np.float32(np.inf)))
        top_true, top_ent = np.sort(tmax[:t1])[::-1][:k], np.sort(m1[:t1])[::-1][:k]
        for j in range(k):
            if top_true[j] >= e1:
                assert _key(top_ent[j]) == _key(top_true[j])
            else:
                assert top_ent[j] < e1
        thr_true = max(thr, _thr(tmax[:t1], k, margin))
        thr_r = _raise(thr, m1[:t1], k, margin)
        assert _bits(thr_r) == _bits(thr_true)
        stats["raised" if thr_r > thr else "kept"] += 1
        stats["short"] += _kth_valid(m1[:t1], k) is None
        e2 = _down_f16(thr_r)
        m = entry_maxima(np.where(seg1, e1, e2))
    else:
        m = entry_maxima(np.full(T, e1))
    top_true, top_ent = np.sort(tmax)[::-1][:k], np.sort(m)[::-1][:k]
    assert np.array_equal(_key(top_ent), _key(top_true))         # every j <= k
    assert _bits(_thr(m, k, margin)) == _bits(_thr(tmax, k, margin))                      # thr2
    for k_part in {k, (k + 3) // 4, 1}:                          # out_part = k_part-th largest - margin / 2
        assert _bits(_thr(m, k_part, margin, np.float32(0.5))) == _bits(_thr(tmax, k_part, margin, np.float32(0.5)))
    stats["neg_zero"] += bool(np.any(np.signbit(top_true) & (top_true == 0)))
    stats["negative"] += bool(top_true[0] < 0)


def _stats():
    return dict(raised=0, kept=0, short=0, neg_zero=0, negative=0)


def test_the_join_on_bits_is_the_float_maximum():
    rng = np.random.default_rng(5)
    vals = np.array([0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, np.float32(65504.0), -np.inf], dtype=np.float32)
    for _ in range(200):
        s = rng.choice(vals, size=int(rng.integers(1, 7)))
        m = _join(1, np.zeros(len(s), dtype=np.int64), s, rng.permutation(len(s)))
        assert _key(m[0]) == _key(s.max())
        assert _bits(m)[0] in set(_bits(s).tolist())            # the bits of one of the scores, never a blend
    assert _bits(_join(1, np.zeros(2, dtype=np.int64), np.array([-0.0, 0.0], dtype=np.float32), [0, 1]))[0] == 0
    assert _join(3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), [])[1] == NINF


def test_random_layouts():
    rng = np.random.default_rng(41)
    stats, runs = _stats(), 0
    for trial in range(60):
        T = int(rng.integers(80, 500))
        k = int(rng.choice([1, 3, 10, 25]))
        if T < 3 * k:
            continue
        score = (rng.standard_normal(T * ROWS) * 0.04).astype(np.float32)
        if trial % 3 == 0:                                      # a short last tile
            score[-int(rng.integers(1, ROWS)):] = -np.inf
        if trial % 4 == 1:                                      # coarse values: ties at the thresholds, zeros of both signs
            score = (np.round(score * 64) / np.float32(64)).astype(np.float32)
        if trial % 4 == 2:                                      # all-negative range
            score = (score - np.float32(0.5)).astype(np.float32)
        if trial % 8 == 5:                                      # nothing above zero, coarse: the top maxima are +-0.0
            score = (-np.abs(np.round(score * 16) / np.float32(16))).astype(np.float32)
            score[rng.integers(0, T * ROWS, 40)] = np.float32(-0.0)
        margin = np.float32(rng.choice([0.0, 1.1e-3, 5e-3]))
        t1 = 0 if trial % 5 == 4 else int(rng.integers(k, T))  # ANY cut with >= k tiles before it, or one launch
        _check(score, T, k, t1, margin, rng, stats)
        runs += 1
    assert runs >= 50 and stats["raised"] >= 20 and stats["negative"] >= 10 and stats["neg_zero"] >= 3, stats


def test_cuts_that_raise_and_cuts_that_do_not():
    rng = np.random.default_rng(43)
    T, k, margin = 404, 10, np.float32(1.1e-3)
    ss = T // (3 * k)
    sampled = np.arange(ss // 2, T, ss)
    base = (rng.standard_normal(T * ROWS) * 0.04).astype(np.float32)
    base[-20:] = -np.inf                                        # the last tile is short
    for shift in (np.float32(0.0), np.float32(-2.0)):           # ... and the same with every score negative
        stats = _stats()
        for t1 in (128, 60, 250, k):
            # fewer than k tiles of segment 1 reach the sample's threshold: k winners in SAMPLED tiles of segment 2 set thr,
            # j < k further ones lie in segment 1 -- the raise keeps thr, the row of entry maxima is short
            for j in (0, 1, k - 1):
                s = base.copy()
                s[rng.choice(sampled[sampled >= t1], size=k, replace=False) * ROWS + 3] = 0.9
                s[rng.choice(t1, size=j, replace=False) * ROWS + 9] = 0.95
                _check(s + shift, T, k, t1, margin, rng, stats)
            # k and more: raised to the final value
            s = base.copy()
            s[rng.choice(t1, size=k, replace=False) * ROWS + 7] = 0.9 + 0.001 * np.arange(k, dtype=np.float32)
            _check(s + shift, T, k, t1, margin, rng, stats)
            # a tie group over both segments at margin 0: the threshold IS the tie value
            s = base.copy()
            n1 = min(15, t1)
            tie = np.concatenate([rng.choice(t1, size=n1, replace=False), rng.choice(np.arange(t1, T), size=30 - n1, replace=False)])
            s[tie * ROWS + 11] = np.float32(0.75)
            _check(s + shift, T, k, t1, np.float32(0.0), rng, stats)
        assert stats["kept"] >= 12 and stats["short"] >= 12 and stats["raised"] >= 4, stats
        assert stats["negative"] == (0 if shift == 0 else stats["kept"] + stats["raised"]), stats
