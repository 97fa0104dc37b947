"""Inputs, reference and a CPU model for the exact top-k select of msr_topk.hip (sel_hist / sel_scan / sel_compact / sel_final),
driven through msr_debug_select on raw score rows.

reference()  the contract, restated plainly: drop NaN and -inf, stable sort by (score descending, index ascending), take k.
model()      the select's CONTROL FLOW on the CPU: 12-bit digit histograms, select_step, the candidate cap, the window clamp,
             the work split and Pk.  It returns the answer, the SelState the streaming passes leave (what msr_debug_select
             exports) and the set of BRANCH TAGS the query took.  tests/test_select_cases.py checks model == reference on
             every case, that every tag is reached, and that each planted MUTATION of the model is caught by some case -- the
             evidence that the GPU comparison (tests/test_gpu_select.py) would notice a kernel that is subtly wrong.

Zeros: the kernel orders -0.0 and +0.0 as ONE key and returns the key's score, so a -0.0 comes back as +0.0.  Scores are
compared by bits everywhere else; where the expected score is a zero the result must be +0.0 (same_scores)."""
import numpy as np

BINS = 4096                 # MSR_SEL_BINS
CAP = 4096                  # MSR_SEL_CAP
STAGE = 1024                # staged matches per workgroup of sel_compact_kernel
PART = 8192                 # elements of a dense row per workgroup
GRID = 2048                 # workgroups of a pass over all queries
WIN_SHIFT = 44

MUTATIONS = {
    "last_score_digit": "the last score digit (f32: 8 bits, f64: 4 bits) is not part of the key",
    "last_index_digit": "the last index digit (8 bits) is not part of the key",
    "clamped_bin_resolved": "a k-th key in a clamped window bin (0 / 4095) is taken as a resolved 20-bit prefix",
    "cap_compare": "the not-done test `superset >= CAP + 1` written as `superset > CAP + 1`: 4097 candidates for 4096 slots",
    "stage_overflow": "matches past the 1024 a workgroup stages are dropped instead of appended directly",
    "tie_descending": "ties broken by descending index (key low part = index instead of ~index)",
}

TAGS = (
    "take_all",             # fewer valid elements than k (or exactly k) at digit 0: everything is emitted
    "done_pass0",           # resolved by the first 12 bits
    "done_pass1",           # resolved by 24 bits
    "row_general",          # > CAP elements share 24 key bits: sel_final_kernel resolves further digits over the row
    "row_last_score_digit",  # ... and the last score digit is what cuts the group
    "row_index_digit",      # ... and an index digit is what cuts the group
    "win_resolved", "win_bin1", "win_bin4094",   # the window pass resolved 20 bits (in bin 1 / 4094: next to the clamps)
    "win_clamp_lo", "win_clamp_hi",              # k-th key in a clamped bin: the general path from scratch
    "win_overflow",         # a window bin with > CAP members: the final kernel resumes at digit 1
    "win_take_all",         # total <= k inside the window pass
    "final_direct",         # done path, candidates <= Pk: sorted as they are
    "final_refine",         # done path, candidates > Pk: further digits resolved on the candidates
    "final_refine_last",    # ... down to digit ND - 1
    "stage_overflow",       # > STAGE matches in one workgroup's range: the direct-append branch of the compaction
    "cap_exact", "cap_plus_one",   # superset of exactly CAP (done) / CAP + 1 (not done)
    "parts_capped", "parts_forced_one",          # 2048 / nq caps the work split; nq > 2048 forces one part
    "list_multi_seg", "list_empty_seg",          # several segments per workgroup; an empty segment
    "index_bit24",          # a selected index >= 2^24
)

STATE_FIELDS = ("pref_hi", "mask_hi", "pref_lo", "mask_lo", "k_rem", "n_above", "done", "n_sel")


# ----------------------------------------------------------------------------------------------------------------- keys
def ord_keys(s):
    """The orderable key of msr_ord32 / msr_ord64 as uint64 (f32: in the low 32 bits)."""
    if s.dtype == np.float32:
        u = s.view(np.uint32).copy()
        u[s == 0] = 0
        return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    u = s.view(np.uint64).copy()
    u[s == 0] = 0
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def digit_pos(sb, d):
    """(part, shift, width) of digit d: ceil(sb / 12) score digits, then 12, 12, 8 bits of ~index."""
    ns = (sb + 11) // 12
    top = sb - 12 * d if d < ns else 32 - 12 * (d - ns)
    width = min(top, 12)
    return (0 if d < ns else 1), top - width, width


def n_digits(sb):
    return (sb + 11) // 12 + 3


# ------------------------------------------------------------------------------------------------------------ reference
def reference(scores, docs, k):
    """scores [m] float, docs [m] int (None: 0 .. m-1) -> (docs, scores) of the k best valid elements."""
    if docs is None:
        docs = np.arange(len(scores), dtype=np.int64)
    ok = ~np.isnan(scores) & (scores != -np.inf)
    s, d = scores[ok], np.asarray(docs, np.int64)[ok]
    if len(s) > 4 * k + 16:                       # (only so that a 16 M row is not sorted whole: everything >= the k-th value)
        thr = np.partition(s, len(s) - k)[len(s) - k]
        keep = s >= thr
        s, d = s[keep], d[keep]
    order = np.lexsort((d, -s))[:k]               # stable; -0.0 == +0.0 compare equal, so zeros go by index
    return d[order], s[order]


def same_scores(got, exp):
    """Bit equality, except that an expected zero of either sign must come back as +0.0."""
    it = np.uint32 if exp.dtype == np.float32 else np.uint64
    e = exp.copy()
    e[exp == 0] = 0.0
    return got.dtype == exp.dtype and got.shape == exp.shape and bool((got.view(it) == e.view(it)).all())


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One msr_debug_select call.  scores [nq, stride]; dense: row q = scores[q, :n]; lists: idx [nq, stride], counts
    [nq, n_seg], seg_stride, win_base (uint64 [nq]) or None; within: set_bits uint32 [n_sets, words], q_set int32 [nq].
    tags: the branches at least one query of the case must take.  big_tie: follow it with a small case on the same engine."""

    def __init__(self, name, scores, k, tags, n=None, idx=None, counts=None, seg_stride=0, win_base=None, set_bits=None,
                 q_set=None, big_tie=False):
        self.name, self.scores, self.k, self.tags = name, np.ascontiguousarray(scores), int(k), frozenset(tags)
        assert self.scores.ndim == 2 and set(tags) <= set(TAGS), name
        self.nq, self.stride = self.scores.shape
        self.n = self.stride if n is None else int(n)
        self.idx, self.counts, self.seg_stride, self.win_base = idx, counts, int(seg_stride), win_base
        self.set_bits, self.q_set, self.big_tie = set_bits, q_set, big_tie
        self.sb = 32 if self.scores.dtype == np.float32 else 64
        if idx is not None:
            assert self.sb == 64 and counts.shape[0] == self.nq and counts.shape[1] * self.seg_stride <= self.stride
            assert (counts <= self.seg_stride).all()

    def parts(self):
        natural = self.counts.shape[1] if self.idx is not None else (self.n + PART - 1) // PART
        return max(1, min(natural, max(GRID // self.nq, 1))), natural

    def row(self, q):
        """-> (scores, docs, part) of the elements query q sees, in row order; part = the workgroup that reads each."""
        parts, _ = self.parts()
        if self.idx is None:
            s = self.scores[q, :self.n]
            d = np.arange(self.n, dtype=np.int64)
            per = (self.n + parts - 1) // parts if self.n else 1
            part = d // max(per, 1)
            if self.q_set is not None:
                v = int(self.q_set[q])
                if v != -1:
                    if v < -1 or v >= self.set_bits.shape[0]:
                        keep = np.zeros(self.n, bool)
                    else:
                        keep = ((self.set_bits[v][d >> 5] >> (d & 31).astype(np.uint32)) & 1).astype(bool)
                    s, d, part = s[keep], d[keep], part[keep]
            return s, d, part
        n_seg = self.counts.shape[1]
        per = (n_seg + parts - 1) // parts
        pos = np.concatenate([np.arange(sg * self.seg_stride, sg * self.seg_stride + int(self.counts[q, sg]))
                              for sg in range(n_seg)] + [np.zeros(0, np.int64)]).astype(np.int64)
        part = (pos // max(self.seg_stride, 1)) // per if self.seg_stride else np.zeros(len(pos), np.int64)
        return self.scores[q, pos], self.idx[q, pos].astype(np.int64), part

    def expected(self, q):
        s, d, _ = self.row(q)
        return reference(s, d, self.k)


# ---------------------------------------------------------------------------------------------------------------- model
class _State:
    def __init__(self, k):
        self.pref_hi = self.mask_hi = self.pref_lo = self.mask_lo = 0
        self.k_rem, self.n_above, self.done, self.n_sel = k, 0, 0, 0

    def copy(self):
        c = _State(0)
        c.__dict__.update(self.__dict__)
        return c

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f in STATE_FIELDS)


def _match(S, hi, lo):
    return ((hi & np.uint64(S.mask_hi)) == np.uint64(S.pref_hi)) & ((lo & np.uint32(S.mask_lo)) == np.uint32(S.pref_lo))


def _at_or_above(S, hi, lo):
    mh = hi & np.uint64(S.mask_hi)
    return (mh > np.uint64(S.pref_hi)) | ((mh == np.uint64(S.pref_hi)) & ((lo & np.uint32(S.mask_lo)) >= np.uint32(S.pref_lo)))


def _digits(sb, d, hi, lo):
    part, shift, width = digit_pos(sb, d)
    src = hi if part == 0 else lo.astype(np.uint64)
    return ((src >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)


def _select_step(h, S, digit, k, sb, win_base, mut, tags):
    """select_step of msr_topk.hip on histogram h; returns the superset count (None: the step changed nothing)."""
    total = int(h.sum())
    if digit <= 0 and total <= S.k_rem:
        S.done, S.n_sel = 1, total
        tags.add("win_take_all" if digit < 0 else "take_all")
        return None
    need = S.k_rem
    suf = np.cumsum(h[::-1])[::-1]                              # suf[b] = elements in bins >= b
    at = np.nonzero(suf >= need)[0]
    if len(at) == 0:                                            # (no thread finds its bin: only a mutated model gets here)
        return None
    b = int(at[-1])
    above = int(suf[b + 1]) if b + 1 < BINS else 0
    superset = S.n_above + above + int(h[b])
    S.n_sel = k
    cap = CAP + 1 if mut == "cap_compare" else CAP
    if superset == CAP:
        tags.add("cap_exact")
    if superset == CAP + 1:
        tags.add("cap_plus_one")
    if digit < 0:
        if (b == 0 or b == BINS - 1) and mut != "clamped_bin_resolved":
            S.done = 0
            tags.add("win_clamp_lo" if b == 0 else "win_clamp_hi")
        else:
            S.pref_hi = ((win_base + b) << WIN_SHIFT) & (2**64 - 1)
            S.mask_hi = (2**64 - 1) << WIN_SHIFT & (2**64 - 1)
            S.n_above += above
            S.k_rem -= above
            if superset <= cap:
                S.done = 1
                tags.add("win_resolved")
                if b in (1, BINS - 2):
                    tags.add("win_bin1" if b == 1 else "win_bin4094")
            else:
                tags.add("win_overflow")
    else:
        part, shift, width = digit_pos(sb, digit)
        if part == 0:
            S.pref_hi |= b << shift
            S.mask_hi |= ((1 << width) - 1) << shift
        else:
            S.pref_lo |= b << shift
            S.mask_lo |= ((1 << width) - 1) << shift
        S.n_above += above
        S.k_rem -= above
        if superset <= cap or digit == n_digits(sb) - 1:
            S.done = 1
    return superset


def _first_open_digit(S, sb):
    for d in range(n_digits(sb)):
        part, shift, _ = digit_pos(sb, d)
        if not ((S.mask_hi if part == 0 else S.mask_lo) >> shift) & 1:
            return d
    return n_digits(sb)


def model_row(scores, docs, part, sb, k, win_base=None, mut=None):
    """One query.  scores / docs / part: what Case.row returns.  -> (docs, scores, state tuple after the streaming passes,
    tags).  Candidates arrive in an order the GPU does not define; the model takes the one least kind to a wrong key:
    descending row position."""
    tags = set()
    ok = ~np.isnan(scores) & (scores != -np.inf)
    s, d, part = scores[ok], docs[ok], part[ok]
    hi = ord_keys(s)
    lo = (~d.astype(np.uint32)) if mut != "tie_descending" else d.astype(np.uint32)
    ns, nd = (sb + 11) // 12, n_digits(sb)
    if mut == "last_score_digit":
        hi = hi & ~np.uint64((1 << digit_pos(sb, ns - 1)[2]) - 1)
    if mut == "last_index_digit":
        lo = lo & ~np.uint32(0xFF)
    S = _State(k)
    window = sb == 64 and win_base is not None
    # ---- streaming passes (sel_hist_kernel + sel_scan_kernel)
    for digit in ([-1] if window else [0, 1]):
        if S.done:
            break
        if digit < 0:
            b = (hi >> np.uint64(WIN_SHIFT)).astype(np.int64) - int(win_base)
            h = np.bincount(np.clip(b, 0, BINS - 1), minlength=BINS)
        else:
            m = _match(S, hi, lo) if digit > 0 else slice(None)
            h = np.bincount(_digits(sb, digit, hi[m], lo[m]), minlength=BINS)
        _select_step(h, S, digit, k, sb, int(win_base) if window else 0, mut, tags)
        if S.done and digit >= 0 and "take_all" not in tags:
            tags.add("done_pass0" if digit == 0 else "done_pass1")
    state = S.as_tuple()
    pk = 64
    while pk < k:
        pk <<= 1
    if S.done:
        # ---- sel_compact_kernel: everything at or above the prefix, per workgroup STAGE staged + the rest appended directly
        sel = np.nonzero(_at_or_above(S, hi, lo))[0]
        cnt_part = np.bincount(part[sel], minlength=1) if len(sel) else np.zeros(1, np.int64)
        if cnt_part.max() > STAGE:
            tags.add("stage_overflow")
            if mut == "stage_overflow":
                rank = np.zeros(len(sel), np.int64)
                for p in np.nonzero(cnt_part > STAGE)[0]:
                    w = np.nonzero(part[sel] == p)[0]
                    rank[w] = np.arange(len(w))
                sel = sel[rank < STAGE]
        sel = sel[:CAP]
        chi, clo = hi[sel], lo[sel]
        cnt = len(sel)
        if cnt <= pk:
            tags.add("final_direct")
            keep = np.arange(cnt)
        else:
            tags.add("final_refine")
            dgt, cur = _first_open_digit(S, sb), cnt
            while cur > pk and dgt < nd:
                m = _match(S, chi, clo)
                sup = _select_step(np.bincount(_digits(sb, dgt, chi[m], clo[m]), minlength=BINS), S, dgt, k, sb, 0, mut, tags)
                cur = cur if sup is None else sup
                if dgt == nd - 1:
                    tags.add("final_refine_last")
                dgt += 1
            keep = np.nonzero(_at_or_above(S, chi, clo))[0]
        sel = sel[keep]
    else:
        # ---- sel_final_kernel finishing the radix select over the row
        d0 = _first_open_digit(S, sb)
        if S.mask_hi:
            tags.add("row_general")
        for dgt in range(d0, nd):
            m = _match(S, hi, lo)
            _select_step(np.bincount(_digits(sb, dgt, hi[m], lo[m]), minlength=BINS), S, dgt, k, sb, 0, mut, tags)
            if S.done:
                if "take_all" not in tags and d0 >= 1:
                    if dgt == ns - 1:
                        tags.add("row_last_score_digit")
                    if dgt >= ns:
                        tags.add("row_index_digit")
                break
        sel = np.nonzero(_at_or_above(S, hi, lo))[0][:CAP]
    order = np.lexsort((lo[sel], hi[sel]))[::-1]                # descending keys; equal (mutated) keys: later position first
    sel = sel[order][:min(S.n_sel, len(sel))]
    if len(sel) and int(d[sel].max()) >= 1 << 24:
        tags.add("index_bit24")
    return d[sel], s[sel] + s.dtype.type(0), state, tags


def model(case, q, mut=None):
    s, d, part = case.row(q)
    wb = None if case.win_base is None else int(case.win_base[q])
    docs, sc, state, tags = model_row(s, d, part, case.sb, case.k, wb, mut)
    parts, natural = case.parts()
    if parts < natural:
        tags.add("parts_forced_one" if case.nq > GRID else "parts_capped")
    if case.idx is not None:
        n_seg = case.counts.shape[1]
        if (n_seg + parts - 1) // parts > 1:
            tags.add("list_multi_seg")
        if (case.counts[q] == 0).any():
            tags.add("list_empty_seg")
    return docs, sc, state, tags


# ------------------------------------------------------------------------------------------------------------- builders
def _bits32(b):
    return np.asarray(b, np.uint32).view(np.float32)


def _bits64(b):
    return np.asarray(b, np.uint64).view(np.float64)


def _specials(dt):
    tiny = np.finfo(dt).tiny
    sub = np.array([1, 2, 3], np.uint32 if dt == np.float32 else np.uint64).view(dt)       # subnormals
    return np.concatenate([np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, tiny, -tiny, -1.5, np.finfo(dt).max,
                                     -np.finfo(dt).max], dt), sub, -sub])


def random_rows(dt, nq, n, seed, special=True, negative=False):
    """Ordinary rows: normal values rounded so that exact ties occur, the special values sprinkled in."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((nq, n)) * 3, 3).astype(dt)
    if negative:
        x = -np.abs(x) - dt(0.25)
    if special and n >= 8:
        sp = _specials(dt)
        for q in range(nq):
            at = rng.choice(n, size=min(n // 2, 3 * len(sp)), replace=False)
            x[q, at] = sp[np.arange(len(at)) % len(sp)]
    return x


def group_row(dt, n, g, above, seed, contiguous_at=None, shared12=True):
    """One row: g elements that agree in the top 24 key bits (f32) / top 60 (f64) and differ only in the last score digit,
    `above` elements higher, the rest lower -- sharing the group's first 12 key bits (shared12) or not."""
    rng = np.random.default_rng(seed)
    if dt == np.float32:
        grp = _bits32(np.uint32(0x3F880000) + rng.integers(0, 256, g).astype(np.uint32))
        low = _bits32(np.uint32(0x3F800000) + rng.integers(0, 0x40000, n).astype(np.uint32)) if shared12 else \
            rng.random(n).astype(dt) * dt(0.5)
    else:
        grp = _bits64(np.uint64(0x3FF0800000000000) + rng.integers(0, 16, g).astype(np.uint64))
        low = _bits64(np.uint64(0x3FF0000000000000) + rng.integers(0, 1 << 45, n).astype(np.uint64)) if shared12 else \
            rng.random(n).astype(dt) * dt(0.5)
    row = low.astype(dt)
    if contiguous_at is None:
        at = rng.choice(n, size=g + above, replace=False)
    else:
        at = np.concatenate([np.arange(contiguous_at, contiguous_at + g), rng.choice(contiguous_at, size=above, replace=False)])
    row[at[:g]] = grp
    row[at[g:]] = dt(2.0) + np.arange(above).astype(dt)
    return row[None, :]


def _list_case(name, nq, n_seg, seg_stride, k, seed, tags, pool=None, win_target=None, empty=True):
    """Lists: per query a pool of (score, document) pairs dealt over the segments in random order, some segments empty, the
    unused slots poisoned with a huge score and an index no row has.  pool(q, rng) -> scores; win_target(q, scores) -> anchor."""
    rng = np.random.default_rng(seed)
    stride = n_seg * seg_stride
    sc = np.full((nq, stride), 1e300)
    ix = np.full((nq, stride), 0x7FFFFFF0, np.int32)
    counts = np.zeros((nq, n_seg), np.int32)
    wb = np.zeros(nq, np.uint64) if win_target else None
    for q in range(nq):
        v = pool(q, rng) if pool else np.round(np.abs(rng.standard_normal(int(rng.integers(0, stride // 2 + 1)))) * 4, 2)
        live = np.ones(n_seg, bool)
        if empty and n_seg > 1:
            live[rng.choice(n_seg, size=max(1, n_seg // 4), replace=False)] = False
        m = min(len(v), int(live.sum()) * seg_stride)
        v = v[:m]
        docs = rng.choice(1 << 22, size=m, replace=False).astype(np.int32)
        slots = np.concatenate([np.arange(sg * seg_stride, (sg + 1) * seg_stride) for sg in np.nonzero(live)[0]])
        seg_of = np.sort(rng.choice(slots, size=m, replace=False)) // seg_stride      # how many land in each segment
        for sg in range(n_seg):
            c = int((seg_of == sg).sum())
            counts[q, sg] = c
        o = 0
        for sg in range(n_seg):
            c = int(counts[q, sg])
            sc[q, sg * seg_stride: sg * seg_stride + c] = v[o:o + c]
            ix[q, sg * seg_stride: sg * seg_stride + c] = docs[o:o + c]
            o += c
        if win_target:
            wb[q] = np.uint64(win_target(q, v))
    return Case(name, sc, k, tags, idx=ix, counts=counts, seg_stride=seg_stride, win_base=wb)


P_ONE = 0xBFF00                                   # the 20-bit key prefix of 1.0 (sign flipped, exponent 0x3FF, 8 mantissa bits)


def _by_prefix(rng, prefixes):
    """positive doubles with the given 20-bit key prefixes and random lower bits"""
    p = np.asarray(prefixes, np.uint64)
    return _bits64(((p & np.uint64(0x7FFFF)) << np.uint64(WIN_SHIFT)) | rng.integers(0, 1 << 44, len(p)).astype(np.uint64))


def _kth_prefix(v, k):
    key = np.sort(ord_keys(np.asarray(v, np.float64)))[::-1]
    return int(key[k - 1] >> np.uint64(WIN_SHIFT))


def _window_cases():
    k = 100

    def spread(q, rng):            # 300 above the k-th region, thousands below, a few per prefix
        return rng.permutation(_by_prefix(rng, P_ONE + rng.integers(-3000, 300, 3500)))

    def heavy(q, rng):             # 5000 elements in ONE prefix, 40 above it
        return rng.permutation(np.concatenate([_by_prefix(rng, np.full(5000, P_ONE)), _by_prefix(rng, P_ONE + 1 + rng.integers(0, 50, 40))]))

    def top_heavy(q, rng):         # 6000 elements over many prefixes, all far above where the bound points
        return rng.permutation(_by_prefix(rng, P_ONE + rng.integers(0, 2000, 6000)))

    mk = lambda name, pool, tgt, tags, kk=k: _list_case(name, 2, 8, 1024, kk, 77, tags, pool=pool, win_target=tgt, empty=False)
    return [
        ("win_bin0_clamped", lambda: mk("win_bin0_clamped", spread, lambda q, v: _kth_prefix(v, k) + 40, {"win_clamp_lo"})),
        ("win_bin0_exact", lambda: mk("win_bin0_exact", spread, lambda q, v: _kth_prefix(v, k), {"win_clamp_lo"})),
        ("win_bin1", lambda: mk("win_bin1", spread, lambda q, v: _kth_prefix(v, k) - 1, {"win_resolved", "win_bin1"})),
        ("win_bin4094", lambda: mk("win_bin4094", spread, lambda q, v: _kth_prefix(v, k) - 4094, {"win_resolved", "win_bin4094"})),
        ("win_bin4095_exact", lambda: mk("win_bin4095_exact", spread, lambda q, v: _kth_prefix(v, k) - 4095, {"win_clamp_hi"})),
        ("win_bound_too_low", lambda: mk("win_bound_too_low", top_heavy, lambda q, v: P_ONE - 4095 - 500, {"win_clamp_hi"})),
        ("win_bin_over_cap", lambda: mk("win_bin_over_cap", heavy, lambda q, v: P_ONE - 2000, {"win_overflow", "row_general"})),
        ("win_total_below_k", lambda: mk("win_total_below_k", lambda q, rng: np.abs(rng.standard_normal(50 + q)) + 1.0,
                                         lambda q, v: P_ONE - 100, {"win_take_all"})),
        ("win_total_equals_k", lambda: mk("win_total_equals_k", lambda q, rng: np.abs(rng.standard_normal(k)) + 1.0,
                                          lambda q, v: P_ONE - 100, {"win_take_all"})),
    ]


def _bitset(mask):
    n = len(mask)
    w = np.zeros((n + 31) // 32, np.uint32)
    i = np.nonzero(mask)[0]
    np.bitwise_or.at(w, i >> 5, (np.uint32(1) << (i & 31).astype(np.uint32)))
    return w


def _within_case():
    n, rng = 20000, np.random.default_rng(41)
    x = random_rows(np.float32, 7, n, 40)
    x[:, 5000:5400] = np.float32(9.5)                         # a tie group at the top of every row ...
    m_tie = np.zeros(n, bool)
    m_tie[5001:5400:2] = True                                 # ... that set 1 holds every other member of
    m_tie[rng.choice(n, 3000, replace=False)] = True
    sets = np.stack([_bitset(rng.random(n) < 0.5), _bitset(m_tie), _bitset(np.zeros(n, bool)), _bitset(np.arange(n) == n - 1)])
    q_set = np.array([-1, 0, 1, 2, 9, -7, 3], np.int32)       # all, ordinary, ties straddling, no bit set, two "none", one document
    return Case("within_mixed_sets", x, 300, {"take_all", "done_pass0"}, set_bits=sets, q_set=q_set)


def _tie200_case():
    x = (np.random.default_rng(8).random((1, 65536)) * 0.5).astype(np.float32)
    at = 512 * 37 + np.sort(np.random.default_rng(9).choice(256, 200, replace=False))
    x[0, at] = 1.0
    return Case("tie200_one_index_block_k10", x, 10, {"done_pass0", "final_refine", "final_refine_last"})


def _big_row_case():
    n = (1 << 24) + 5000
    x = np.zeros((1, n), np.float32)
    x[0, ::3] = -0.0
    x[0, 1 << 24:] = 1.0                                      # 5000 equal scores behind index 2^24
    x[0, 12345] = np.inf
    return Case("row_above_2p24_ties_behind_bit24", x, 10, {"row_general", "row_index_digit", "index_bit24"}, big_tie=True)


def _stage_case(dt):
    x = group_row(dt, 5 * PART, 3000, 0, 61, contiguous_at=2 * PART + 100, shared12=False)
    order = np.argsort(x[0, 2 * PART + 100: 2 * PART + 3100], kind="stable")
    x[0, 2 * PART + 100: 2 * PART + 3100] = x[0, 2 * PART + 100: 2 * PART + 3100][order]     # the best stand last in the run
    return Case(f"stage_overflow_{dt.__name__}", x, 1000, {"stage_overflow", "done_pass0", "final_refine"})


def _cap_last_case():
    """4097 candidates of which the one at the highest position is the best: what a 4096-slot buffer filled in row order loses"""
    x = group_row(np.float32, 40000, 4097, 0, 67)
    at = np.nonzero(x[0] >= _bits32(np.uint32(0x3F880000)))[0]
    x[0, at] = _bits32(np.uint32(0x3F880000))
    x[0, at[-1]] = _bits32(np.uint32(0x3F8800FF))
    return Case("group_4097_best_is_last", x, 10, {"cap_plus_one", "row_general"}, big_tie=True)


def _build_cases():
    c = []
    add = lambda name, fn: c.append((name, fn))
    for dt in (np.float32, np.float64):
        t = dt.__name__
        for n in (1, 63, 64, 65, 8191, 8192, 8193, 4 * PART + 1, 300001):
            k = {1: 1, 63: 63, 64: 64, 65: 65, 8191: 100, 8192: 1000, 8193: 1023, 4 * PART + 1: 1024, 300001: 2}[n]
            tags = {"take_all"} if n <= 65 else set()
            add(f"random_{t}_n{n}_k{k}", lambda dt=dt, n=n, k=k, tags=tags: Case(f"random_{dt.__name__}_n{n}_k{k}",
                                                                                  random_rows(dt, 3, n, n + k), k, tags))
        for k in (1, 2, 63, 64, 65, 100, 1000, 1023, 1024):
            add(f"random_{t}_n20000_k{k}", lambda dt=dt, k=k: Case(f"random_{dt.__name__}_n20000_k{k}",
                                                                    random_rows(dt, 2, 20000, 500 + k), k, set()))
        add(f"negatives_{t}", lambda dt=dt: Case(f"negatives_{dt.__name__}", random_rows(dt, 2, 9000, 3, special=False, negative=True),
                                                 100, {"done_pass0"}))

        def kth_negative(dt=dt):
            x = random_rows(dt, 2, 9000, 4, special=False, negative=True)
            x[:, :50] = np.abs(x[:, :50])
            return Case(f"kth_among_negatives_{dt.__name__}", x, 100, set())
        add(f"kth_among_negatives_{t}", kth_negative)

        def valid_count(dt=dt, extra=0):
            x = np.full((3, 700), np.nan, dt)
            x[:, 1::2] = -np.inf
            x[0, 5:305:3] = np.round(np.random.default_rng(5).standard_normal(100), 2).astype(dt)      # 100 valid elements
            x[1, 9] = dt(-0.0)                                                                         # one valid element
            return Case(f"k_vs_valid_{dt.__name__}_{extra}", x, 100 + extra, {"take_all", "final_direct"})   # row 2: none valid
        add(f"k_equals_valid_{t}", valid_count)
        add(f"k_above_valid_{t}", lambda dt=dt, f=valid_count: f(dt, 1))
        add(f"zeros_and_subnormals_{t}", lambda dt=dt: Case(f"zeros_and_subnormals_{dt.__name__}", np.tile(np.concatenate(
            [_specials(dt)[2:], np.zeros(40, dt), -np.zeros(40, dt)])[None, :], (2, 1)), 64, {"final_refine_last"}))
        for g in (4096, 4097, 5000, 70000):
            for k in (10, 1000):
                tags = {"cap_exact", "done_pass1"} if g == 4096 else {"row_general"} | ({"cap_plus_one"} if g == 4097 else set())
                if g > 4096:
                    tags |= {"row_index_digit"} if (g == 70000 and dt == np.float64) else {"row_last_score_digit"}
                add(f"group_{t}_{g}_k{k}", lambda dt=dt, g=g, k=k, tags=tags: Case(
                    f"group_{dt.__name__}_{g}_k{k}", group_row(dt, max(3 * g, 40000), g, 0, g + k), k, tags, big_tie=g > 4096))
        add(f"group_{t}_4093_above3", lambda dt=dt: Case(f"group_{dt.__name__}_4093_above3", group_row(dt, 40000, 4093, 3, 11), 100,
                                                         {"cap_exact", "done_pass1", "final_refine"}))
        add(f"group_{t}_4094_above3", lambda dt=dt: Case(f"group_{dt.__name__}_4094_above3", group_row(dt, 40000, 4094, 3, 12), 100,
                                                         {"cap_plus_one", "row_general", "row_last_score_digit"}, big_tie=True))
        add(f"stage_overflow_{t}", lambda dt=dt: _stage_case(dt))
        add(f"all_equal_{t}_70000", lambda dt=dt: Case(f"all_equal_{dt.__name__}_70000", np.full((2, 70000), 0.25, dt), 1000,
                                                       {"row_general", "row_index_digit"}, big_tie=True))
    add("group_4097_best_is_last", _cap_last_case)
    add("tie200_one_index_block_k10", _tie200_case)
    add("row_above_2p24", _big_row_case)
    add("nq5_n300001", lambda: Case("nq5_n300001", random_rows(np.float32, 5, 300001, 21), 100, {"done_pass0"}))
    add("nq1100_n8193_parts_capped", lambda: Case("nq1100_n8193_parts_capped", random_rows(np.float32, 1100, 8193, 22), 10,
                                                  {"parts_capped"}))
    add("nq2100_parts_forced_one", lambda: Case("nq2100_parts_forced_one", random_rows(np.float64, 2100, 8200, 23), 10,
                                                {"parts_forced_one"}))
    add("within_mixed_sets", _within_case)
    for n_seg in (1, 2, 8, 64):
        add(f"list_nseg{n_seg}", lambda n_seg=n_seg: _list_case(f"list_nseg{n_seg}", 3, n_seg, 8192 // n_seg, 100, 90 + n_seg,
                                                                 {"list_empty_seg"} if n_seg > 1 else set()))
    add("list_nseg64_nq300", lambda: _list_case("list_nseg64_nq300", 300, 64, 64, 37, 95, {"list_multi_seg", "list_empty_seg", "parts_capped"}))
    add("list_ties_over_cap", lambda: _list_case("list_ties_over_cap", 2, 8, 2048, 1000, 96, {"row_general", "row_index_digit"},
                                                 pool=lambda q, rng: np.full(9000, 2.5)))
    c.extend(_window_cases())
    return c


CASES = _build_cases()                            # (name, builder): rows are built on demand (the largest is 67 MB)
SMALL_AFTER = "random_float32_n8193_k1023"        # the ordinary case run behind every big_tie case on the same engine
MAX_QUERIES = 2304                                # the engine the GPU test makes: nq = 2100 > 2048 fits (msr_create takes <= 4096)


def build(name):
    return dict(CASES)[name]()
