"""Every engine entry point on a caller's stream, behind pending work (tests/stream_cases.py: the side stream, the delay, the
stage, the table).

1  the side stream does not wait for the null stream (its flags, read back) and the hardware runs it beside the null stream
   (the positive control), at the start of the module and again at its end.
2  every probe of the call-sequence catalogue, and the dirtiers that leave through a fallback with further launches, on an
   engine created, bound and used on the side stream, its inputs written behind the delay: the outputs pass the CPU oracles
   of test_gpu_call_sequences.py part A, equal the default-stream bytes of the same entry, differ from what the decoy
   inputs give, and scratch_dirty() is clean.  The first call on every fresh engine is select_f32: it reads the two buffers
   msr_create clears.
3  at the return of every engine method the event behind the delay is pending (enqueue-only) or done (synchronising), as
   stream_cases.TABLE says; the calls of bench.py's timed step are all enqueue-only.
4  two engines on two streams, the shape `bench.py --pipelined` runs: BM25 of the next batch on the side stream beside the
   dense finish chain, gather and fuse of this one on the main stream; equal to the serial run byte for byte, with and without
   the delay on the side stream, and at RERANK_BAR of the CPU chain.
"""
import copy
import time

import numpy as np
import pytest
import torch

import call_sequence_cases as cs
import stream_cases as sx
import test_gpu_call_sequences as seq

pytestmark = pytest.mark.gpu

T0 = [None]
TIMES = {}                                                    # (bundle, entry) -> ms from the sleep to the last method's return
OBSERVED = {}                                                 # method -> {kind observed: an entry that showed it}


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    T0[0] = time.time()
    s = sx.SideStream(torch, torch.device("cuda", 0))         # (the control at the start of the module: raises if no stream serves)
    print(f"side stream {s.stream.cuda_stream:#x}: {s.cycles_per_ms:.0f} sleep cycles per ms, delay {sx.DELAY_MS} ms, "
          f"streams tried: {s.tried}")
    yield s
    s.close()
    enq = sorted(TIMES.values())
    if enq:
        print(f"enqueue times behind the delay (entries that are enqueue-only throughout): longest {enq[-1]:.2f} ms, median "
              f"{enq[len(enq) // 2]:.2f} ms; longest five: {sorted(TIMES.items(), key=lambda kv: -kv[1])[:5]}")
    print(f"test_gpu_streams.py: {time.time() - T0[0]:.1f} s wall")


class _Staged:
    """The four bundles on the side stream, each with the default-stream bytes of its entries (from an engine of its own on
    the default stream, closed again) and the staged run of select_f32 as the FIRST call of its engine."""

    def __init__(self, side):
        self.side, self.b, self.results = side, {}, {}

    def get(self, name):
        if name not in self.b:
            t0 = time.time()
            ref = seq._Bundles()
            rb = ref.get(name)                                # default stream: every probe as the first call after a fresh bind
            clean, ref_out = rb.clean, {}
            for e in sx.entries_on_stream(name):
                if e.kind == "dirtier":
                    rb.fresh()
                    ref_out[e.name], _ = e.run(rb)
            ref.close()
            with torch.cuda.stream(self.side.stream):
                b = sx.StagedBundle(name, torch)
                b.clean, b.ref_out = clean, ref_out
                assert b.eng.calls == 0
                first = sx.entries_on_stream(name)[0]
                assert first.name == "select_f32"
                self.results[(name, first.name)] = sx.run_on_stream(b, first, self.side)
            self.b[name] = b
            print(f"bundle {name} on the side stream: reference engine, staged engine and first select in {time.time() - t0:.1f} s")
        return self.b[name]

    def result(self, name, entry):
        b = self.get(name)
        if (name, entry.name) not in self.results:
            with torch.cuda.stream(self.side.stream):
                self.results[(name, entry.name)] = sx.run_on_stream(b, entry, self.side)
        return b, self.results[(name, entry.name)]

    def close(self):
        for b in self.b.values():
            b.close()


@pytest.fixture(scope="module")
def staged(side):
    s = _Staged(side)
    yield s
    s.close()


# ------------------------------------------------------------------------------------------------------------ 1
def test_the_side_stream_runs_beside_the_null_stream(side):
    assert sx.stream_flags(side.hip, side.stream.cuda_stream) & sx.HIP_STREAM_NON_BLOCKING
    assert side.tried[-1][1] and len(side.tried) <= sx.SideStream.TRIES
    assert side.null_control == (True, True, True), side.null_control
    assert sx.stream_flags(side.hip, side.block.cuda_stream) & sx.HIP_STREAM_NON_BLOCKING == 0
    assert sx.DELAY_MS <= sx.DELAY_CAP_MS
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side.stream):                      # the calibration: the delay lasts what it is meant to last
        a.record()
        side.sleep()
        b.record()
    b.synchronize()
    ms = a.elapsed_time(b)                                    # (the spin counts shader clocks: the length moves with the clock)
    assert sx.MARGIN * sx.LONGEST_ENQUEUE_MS <= ms <= sx.DELAY_CAP_MS, ms
    print(f"the delay of {sx.DELAY_MS} ms lasted {ms:.1f} ms")


# ------------------------------------------------------------------------------------------------------------ 2, 3
CASES = [(bn, e.name) for bn in cs.ALL for e in sx.entries_on_stream(bn)]


def _entry(name):
    return sx.SPLIT_WITH_BOUND if name == sx.SPLIT_WITH_BOUND.name else cs.by_name(name)


def _check_entry(b, entry, res):
    out, rep, decoy_out, kinds, ms, used, stray, conclusive = res
    what = f"bundle {b.name}, {entry.name} on the side stream behind the delay"
    # nothing was launched on the null stream (held back by a sleeping blocking stream while the entry ran)
    assert conclusive, f"{what}: the entry outlasted the {sx.SideStream.HOLD_MS} ms for which the null stream was held"
    assert not stray, f"{what}: work was enqueued on the NULL stream, not on the caller's (it was still pending behind the " \
                      f"blocking stream when the entry had read its outputs from the side stream)"
    # the oracles of part A / the dirtier's own path predicate
    if entry.kind == "probe":
        seq.ORACLES[entry.name](b, entry.name, out)
        if entry.name in seq.EXPECTED_PATH:
            assert rep["dense_path"] == seq.EXPECTED_PATH[entry.name], (what, rep)
        ref = b.clean[entry.name]
    else:
        try:
            entry.check(b, out, rep)
        except AssertionError as e:
            raise AssertionError(f"{what}: the path predicate does not hold: {e}") from e
        ref = b.ref_out[entry.name]
    # byte-equal to the default stream
    bad = seq._diff(out, ref)
    assert not bad, f"{what}: outputs {bad} differ from the default-stream bytes " \
                    f"({seq._where(out, ref, bad[0]) if '.' not in bad[0] else ''})"
    # not the decoy's result
    if entry.name in sx.HOST_INPUT_PROBES:
        assert not seq._diff(decoy_out, out) and not used
    else:
        assert used, f"{what}: no staged input"
        assert seq._diff(decoy_out, out), f"{what}: the decoy inputs give the same bytes as the real ones: a stray read of " \
                                          f"the decoy could not show"
    # the table
    for m, kind in kinds:
        assert m in sx.TABLE, f"{what}: {m} is not in stream_cases.TABLE"
        OBSERVED.setdefault(m, {}).setdefault(kind, f"{b.name}/{entry.name}")
        assert sx.TABLE[m].kind == kind, \
            f"{what}: {m} was {kind} (the event behind the {sx.DELAY_MS} ms delay was " \
            f"{'pending' if kind == sx.ENQ else 'done'} when it returned, {ms:.2f} ms after the sleep was launched); " \
            f"stream_cases.TABLE says {sx.TABLE[m].kind}"
    if kinds and all(k == sx.ENQ for _, k in kinds):
        TIMES[(b.name, entry.name)] = ms
        assert sx.MARGIN * ms <= sx.DELAY_CAP_MS, f"{what}: {ms:.2f} ms to enqueue: no delay under the cap has the margin"


@pytest.mark.parametrize("bundle,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_entry_on_the_side_stream(staged, bundle, name):
    entry = _entry(name)
    b, res = staged.result(bundle, entry)
    _check_entry(b, entry, res)
    with torch.cuda.stream(staged.side.stream):
        seq._assert_clean_scratch(b, entry.name, "on the side stream", entry.pending)


def _observe(b, side, fn):
    """fn(engine) behind one delay on the current stream -> [(method, kind)]"""
    ev = torch.cuda.Event()
    side.sleep()
    ev.record()
    b.eng.event, b.eng.seen = ev, []
    try:
        fn(b.eng)
    finally:
        seen, b.eng.event = b.eng.seen, None
    torch.cuda.current_stream().synchronize()
    return [(m, sx.ENQ if after else sx.SYNC) for m, before, after, _ in seen if before]


def test_the_table_equals_what_the_gpu_shows(staged):
    """Every row of the table marked `seen` is observed with its kind: by the entries above (run here if they have not been),
    and, for the methods no entry calls behind the delay, directly."""
    for bn, name in CASES:
        entry = _entry(name)
        b, res = staged.result(bn, entry)
        _check_entry(b, entry, res)
    side = staged.side
    hyb, bf16, lex = staged.get("hyb"), staged.get("bf16"), staged.get("lex")
    q16 = [lex.inp.queries[i] for i in lex.inp.mixed16]
    sets = [lex.docset(s) for s in lex.inp.within_names(16)]
    direct = [
        (hyb, lambda e: (e.dense_path(), e.scan_width(), e.bm25_split(16), e.dense_split_max(cs.K_DENSE), e.doc_signatures())),
        (hyb, lambda e: e.bind_signatures(None)),
        (bf16, lambda e: (e.batch_width(), e.batch_gemm_ok())),
        (hyb, lambda e: e.gather_rows(hyb.dev("rows_0_5", lambda: np.arange(6, dtype=np.int32)))),
        (hyb, lambda e: e.scratch_dirty()),
        (lex, lambda e: e.pack_queries(q16)),
        (lex, lambda e: e.pack_within(sets, 16)),
    ]
    with torch.cuda.stream(side.stream):
        for b, fn in direct:
            if b is hyb:
                b.dev("rows_0_5", lambda: np.arange(6, dtype=np.int32))      # (uploaded before the delay)
                b.stage.load("real")
            for m, kind in _observe(b, side, fn):
                OBSERVED.setdefault(m, {}).setdefault(kind, f"{b.name}/direct")
                assert sx.TABLE[m].kind == kind, f"{m} called directly on bundle {b.name}: {kind}; the table says {sx.TABLE[m].kind}"
            seq._assert_clean_scratch(b, "direct calls", "on the side stream", 0)
    for r in sx.TABLE.values():
        if r.seen:
            assert set(OBSERVED.get(r.method, {})) == {r.kind}, (r.method, r.kind, OBSERVED.get(r.method))
    for m in OBSERVED:
        assert sx.TABLE[m].seen, f"{m} is observed ({OBSERVED[m]}): mark its row seen"
    for m in sx.HOT_PATH:                                     # the timed step of bench.py: enqueue-only, observed
        assert set(OBSERVED[m]) == {sx.ENQ}, (m, OBSERVED[m])


# ------------------------------------------------------------------------------------------------------------ 4
Q2, K1, K2, BATCHES = 65, 100, 10, 3


class _Pair:
    """Engine A (the whole hyb index) on the main stream, engine B (postings only) on the side stream, three batches."""

    def __init__(self, side):
        from msretr.engine import DeviceEngine
        from msretr.synthetic import synthetic_queries
        from oracle_engine import OracleEngine
        self.side, inp = side, cs.hyb_inputs()
        self.ix = inp.ix
        self.dev = torch.device("cuda", 0)
        terms, qvec = synthetic_queries(self.ix, Q2 * BATCHES, seed=61, device="cpu", lo_rank=5, hi_rank=3000)
        self.A = DeviceEngine(self.ix, max_queries=128, max_k=K1, rerank_max_docs=K1)
        lex_only = copy.copy(self.ix)
        lex_only.emb = None
        with torch.cuda.stream(side.stream):
            self.B = DeviceEngine(lex_only, max_queries=Q2, max_k=K1, rerank_max_docs=0)
            self.packed = [self.B.pack_queries([list(t) for t in terms[i * Q2:(i + 1) * Q2]]) for i in range(BATCHES)]
        self.qv_host = [qvec[i * Q2:(i + 1) * Q2].numpy().copy() for i in range(BATCHES)]
        self.qv = [torch.from_numpy(q).to(self.dev) for q in self.qv_host]
        assert self.A.dense_split_max(K2) >= Q2
        torch.cuda.synchronize(self.dev)
        self.oracle = OracleEngine(self.ix)
        self.serial = self.run("serial")
        self.cpu = None

    def run(self, mode):
        """mode "serial": every call alone, the device drained after it; "plain": bench.py's pipelined loop; "delayed": the
        same with the delay in front of every BM25 stage on the side stream, so that A's chain runs ahead of B's.
        -> per batch the host arrays of (B's lists, A's dense lists, A's fused lists)"""
        A, B, S, dev = self.A, self.B, self.side.stream, self.dev
        main = torch.cuda.current_stream(dev)
        serial = mode == "serial"
        drain = (lambda: torch.cuda.synchronize(dev)) if serial else (lambda: None)

        def stage1(i):                                        # -> (lists, event); enqueued on the side stream
            with torch.cuda.stream(S):
                if mode == "delayed":
                    self.side.sleep()
                lists = B.bm25_topk(None, k=K1, packed=self.packed[i])
                ev = torch.cuda.Event()
                ev.record(S)
            for t in lists:                                   # (allocated on the side stream, read on the main one)
                t.record_stream(main)
            drain()
            return lists, ev

        outs = []
        pend = stage1(0)
        for i in range(BATCHES):
            qv = self.qv[i]
            lists, ev = pend
            A.dense_begin(qv, k=K2, k_part=K2)
            drain()
            behind = torch.cuda.Event()
            behind.record(main)
            S.wait_event(behind)                              # the BM25 stage of the next batch: behind the dense pass
            if i + 1 < BATCHES:
                pend = stage1(i + 1)
            d = A.dense_end(Q2, k=K2, bound=None)
            drain()
            main.wait_event(ev)
            cos, meta = A.rerank_gather(qv, lists[0], lists[2])
            drain()
            r = A.rerank_fuse(lists[0], lists[1], lists[2], cos, meta)
            drain()
            outs.append((lists, d, r))
        main.wait_stream(S)
        torch.cuda.synchronize(dev)
        assert A.dense_path() == 128                          # the streaming pass ran
        return [tuple([x.cpu().numpy() for x in part] for part in o) for o in outs]

    def cpu_chain(self):
        if self.cpu is None:
            import hybrid_ref as H
            from msretr.engine import RERANK_DEFAULTS
            self.cpu = []
            for i, (lists, _, _) in enumerate(self.serial):
                f = H.fused(self.oracle, lists[0], lists[1], lists[2], self.qv_host[i], smoothing=RERANK_DEFAULTS["smoothing"])
                self.cpu.append([np.asarray(x) for x in f])
        return self.cpu

    def close(self):
        self.A.close()
        self.B.close()


@pytest.fixture(scope="module")
def pair(side):
    p = _Pair(side)
    yield p
    p.close()


@pytest.mark.parametrize("mode", ["plain", "delayed"])
def test_two_engines_on_two_streams_equal_the_serial_run(pair, mode):
    got = pair.run(mode)
    for i, (g, s) in enumerate(zip(got, pair.serial)):
        for part, name in enumerate(("bm25", "dense", "fused")):
            for j, (x, y) in enumerate(zip(g[part], s[part])):
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), \
                    f"{mode}: batch {i}, {name} output {j} differs from the serial run of the same calls"
    for i, (g, want) in enumerate(zip(got, pair.cpu_chain())):
        f = g[2]
        assert (g[0][2] > 0).any() and (f[4] > 0).any()
        seq._lists_at_bar(f"{mode}: batch {i} fused", f[0], f[1], f[4], want[0], want[1], want[4], exact_order=False)
    d = pair.A.scratch_dirty()
    assert all(d[x] in (0, -1) for x in seq.COUNTED) and d["split_pending"] == 0, d
    with torch.cuda.stream(pair.side.stream):                 # (B lives on the side stream)
        d = pair.B.scratch_dirty()
    assert all(d[x] in (0, -1) for x in seq.COUNTED) and d["split_pending"] == 0, d


# ------------------------------------------------------------------------------------------------------------ 1, again
def test_the_control_still_holds_at_the_end(side, staged):
    assert side.control(), "at the end of the module work behind the sleeping side stream was visible to the default " \
                           "stream: the window was not open for the tests above"
    assert side.control_null() == (True, True, True), "at the end of the module the held null stream could not be watched"
