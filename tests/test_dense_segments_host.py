"""The segmented emit pass of the streaming dense scan (msr_gemm_f32_pass), restated in numpy.

The pass emits over the first T1 row tiles with the sample's threshold thr, raises the threshold to
thr' = max(thr, k-th largest of those T1 tile maxima - margin) and emits over the remaining tiles with thr'; the bucket then
keeps the entries at or above thr2 = (k-th largest of ALL tile maxima) - margin.  Checked here, on random tile maxima and on
adversarial placements of the winners, for random T1:

* thr <= thr' <= thr2 (the k-th largest over a subset of the tiles is <= the k-th largest over a superset; one margin);
* {entries >= thr in segment 1} u {entries >= thr' in segment 2}, filtered by thr2, is the set {entries >= thr}, filtered
  by thr2 -- what the one-launch pass hands to the finish.

The 256-query kernel compares against the threshold rounded DOWN to f16; the restatement does the same (rounding down is
monotone, so the order of the thresholds survives it)."""
import math
import subprocess

import numpy as np

from test_stream_plan import build_stream_plan_check

ROWS = 32                                                       # rows per tile of the model corpus


def _down_f16(x):
    """Largest f16 <= x (x finite, f32), as the kernel's down_h."""
    h = np.float32(x).astype(np.float16)
    if np.float32(h) > np.float32(x):
        h = np.nextafter(h, np.float16(-np.inf))
    return np.float32(h)


def _kth(v, k):
    return np.sort(v)[-k]


def pass_shape(T, k, grid):
    """The rule of msr_stream_plan.h's pass_shape: (ss, n_s, T1) with T1 = 0 for a one-launch pass."""
    ss = min(64, max(1, T // (3 * k)))
    n_s = (T - ss // 2 + ss - 1) // ss
    t1 = int(math.floor(math.sqrt(T * n_s) / grid + 0.5)) * grid
    if t1 >= max(grid, 2 * k) and T - t1 >= grid:
        return ss, n_s, t1
    return ss, n_s, 0


def _check(score, T, k, t1, margin, f16_thr):
    """score: [T * ROWS] filter scores (-inf: a row behind a short tile)."""
    tmax = score.reshape(T, ROWS).max(axis=1)
    ss = min(64, max(1, T // (3 * k)))
    sample = tmax[ss // 2::ss]
    assert len(sample) >= k
    thr = np.float32(_kth(sample, k) - margin)
    thr_r = max(thr, np.float32(_kth(tmax[:t1], k) - margin))
    thr2 = np.float32(_kth(tmax, k) - margin)
    assert thr <= thr_r <= thr2
    e1, e2 = (_down_f16(thr), _down_f16(thr_r)) if f16_thr else (thr, thr_r)
    assert e1 <= e2 <= thr2
    seg1 = np.arange(T * ROWS) < t1 * ROWS
    one = score >= e1                                           # the one-launch pass
    two = (seg1 & (score >= e1)) | (~seg1 & (score >= e2))      # the segmented pass
    assert not np.any(two & ~one)                               # only ever fewer entries
    keep = score >= thr2                                        # the bucket
    assert np.array_equal(one & keep, two & keep)
    assert np.array_equal(two & keep, keep)                     # ... and nothing at or above thr2 is missing
    return int(one.sum()), int(two.sum()), thr_r


def test_segment_rule_at_the_documented_shapes():
    assert pass_shape(3 * 256 + 40, 10, 256) == (26, 31, 256)            # the GPU test's main shape: 256 + 552 tiles
    ss, n_s, t1 = pass_shape(20100, 100, 256)                            # ~5 M rows, k = 100: the sample stride is capped
    assert (ss, n_s) == (64, 314) and t1 % 256 == 0 and abs(t1 - math.sqrt(20100 * n_s)) <= 128
    assert t1 == 2560
    assert pass_shape(950, 100, 256) == (3, 317, 512)                    # (the ~950-tile corpus of tests/test_gpu_parity.py)
    assert pass_shape(400, 10, 256)[2] == 0                              # sqrt(T n_s) is nearer to 0 rounds than to one
    assert pass_shape(300, 100, 256)[2] == 0                             # no whole round left behind the first
    assert pass_shape(255, 10, 256)[2] == 0
    for T in (512, 808, 5000, 20100, 40000):
        for k in (1, 10, 100, 250):
            if T < 2 * k:
                continue
            t1 = pass_shape(T, k, 256)[2]
            assert t1 == 0 or (t1 % 256 == 0 and t1 >= max(256, 2 * k) and T - t1 >= 256)


def test_the_restatement_is_the_rule_the_pass_runs(tmp_path):
    """pass_shape of csrc/msr_stream_plan.h, printed by tests/stream_plan_check.cpp case by case, equals the restatement above
    on every case: both take the correctly rounded double square root of the same integer product (< 2^53), so no tolerance."""
    r = subprocess.run([build_stream_plan_check(tmp_path), "shapes"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    seen = set()
    for line in r.stdout.splitlines():
        (T, k, grid, single), (ss, n_s, n_seg, t1) = [[int(x) for x in part.split()] for part in line.split(":")]
        want = pass_shape(T, k, grid)
        if single:
            want = want[:2] + (0,)
        assert (ss, n_s, t1) == want and n_seg == (2 if t1 else 1), line
        seen.add((T, k, grid, single))
    Ts = list(range(1, 1201)) + [5000, 20100, 40000, 200000]
    assert seen == {(T, k, grid, single) for T in Ts for k in (1, 3, 10, 25, 100, 250, 1000) if T >= 2 * k
                    for grid in (8, 64, 250, 256, 304) for single in (0, 1)}
    assert any(t for t in seen if pass_shape(*t[:3])[2])            # (the enumeration cuts some passes)


def test_segmented_emission_keeps_what_the_bucket_keeps():
    rng = np.random.default_rng(23)
    fewer = 0
    for trial in range(40):
        T = int(rng.integers(80, 900))
        k = int(rng.choice([1, 3, 10, 25]))
        if T < 3 * k:
            continue
        score = (rng.standard_normal(T * ROWS) * 0.04).astype(np.float32)
        if trial % 3 == 0:                                      # a short last tile
            score[-int(rng.integers(1, ROWS)):] = -np.inf
        if trial % 4 == 1:                                      # coarse values: many exact ties at the thresholds
            score = np.round(score * 64) / np.float32(64)
        t1 = int(rng.integers(k, T))                            # ANY cut with >= k tiles before it is valid
        margin = np.float32(rng.choice([0.0, 1.1e-3, 5e-3]))
        n1, n2, _ = _check(score, T, k, t1, margin, f16_thr=bool(trial & 1))
        fewer += n2 < n1
    assert fewer >= 20                                          # (the refresh does something on most of them)


def test_adversarial_placements_of_the_winners():
    rng = np.random.default_rng(29)
    T, k, margin = 808, 10, np.float32(1.1e-3)
    base = (rng.standard_normal(T * ROWS) * 0.04).astype(np.float32)
    base[-20:] = -np.inf                                        # the last tile is short
    for t1 in (256, 100, 700, k):
        seg1_tiles = rng.choice(t1, size=min(k, t1), replace=False)
        # all winners inside segment 1: the refreshed threshold equals the final one
        s = base.copy()
        s[seg1_tiles * ROWS + 7] = 0.9 + 0.001 * np.arange(len(seg1_tiles), dtype=np.float32)
        if len(seg1_tiles) == k:
            _, _, thr_r = _check(s, T, k, t1, margin, True)
            assert thr_r == np.float32(_kth(s.reshape(T, ROWS).max(axis=1), k) - margin)
        # all inside segment 2: the refresh barely moves the threshold, everything is emitted with the sample's
        s = base.copy()
        s[rng.choice(np.arange(t1, T), size=k, replace=False) * ROWS + 3] = 0.9
        _check(s, T, k, t1, margin, True)
        # a tie group of 30 identical values over both segments, k = 10: every threshold sits margin below the tie value
        s = base.copy()
        n1 = min(15, t1)
        tie = np.concatenate([rng.choice(t1, size=n1, replace=False), rng.choice(np.arange(t1, T), size=30 - n1, replace=False)])
        s[tie * ROWS + 11] = np.float32(0.75)
        for m in (margin, np.float32(0.0)):                     # (margin 0: the threshold IS the tie value -- >= keeps the ties)
            _, n2, _ = _check(s, T, k, t1, m, True)
            assert n2 >= 30
        # the best row is the last valid row of the last, short tile
        s = base.copy()
        s[T * ROWS - 21] = 0.95
        _check(s, T, k, t1, margin, True)
