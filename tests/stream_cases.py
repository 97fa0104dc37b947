"""The engine on a caller's stream (test_stream_cases.py on the CPU, test_gpu_streams.py on the GPU).

include/msretr.h: "`stream` is a hipStream_t ... One engine per (device, stream)".  Every other test of the suite calls the
engine on torch's default stream, which is ordered against everything: a launch that lands on the null stream instead of the
caller's, an input read before the caller's stream has produced it, a scratch clear on the wrong stream -- all return the
right bytes there.  The tests here make such work VISIBLE:

SIDE STREAM   a stream S that does not wait for the null stream (hipStreamNonBlocking, read back with hipStreamGetFlags, not
              assumed) and that the hardware really runs beside it (the positive control: while S sleeps, a write enqueued on S
              behind the sleep is not seen by a default-stream read; with both streams on one hardware queue it would be, and
              every check below would pass vacuously).
DELAY         torch.cuda._sleep, a bounded spin kernel, at the head of S (calibrated once with two events; DELAY_MS).
STAGE         every device input of a catalogue entry (call_sequence_cases.Bundle.dev / _up / qdev, and the host arrays, term
              lists and document sets an entry hands to an engine method) lives three times on the device: REAL, DECOY (the
              same input rotated by one query: valid data, another answer) and LIVE, the tensor the call reads.  A run is:
              LIVE <- DECOY, the entry once, synchronised; then on S: sleep, record E, LIVE <- REAL (device-to-device copies
              behind the sleep), the entry again; at the return of every engine method E.query() is noted.  Work that does not
              wait for S reads decoys or stale intermediates and computes a WRONG ANSWER FROM VALID DATA; nothing can touch a
              bad address.
NULL HELD     while the entry runs behind the delay a BLOCKING stream sleeps too: the null stream waits for it, the side stream
              does not.  A launch that strays to the null stream is then still pending when the entry has read its outputs
              (an event on a second blocking stream stays behind it), whether or not a result depends on it -- the BM25 plan
              kernel's products, for one, change no result (SideStream.hold_null; with a control of its own).
TABLE         what every public DeviceEngine method does to the caller's stream: ENQ (E still pending at the return: the whole
              call was enqueued while the delay ran) or SYNC (E done at the return), with the reason and the C entry points.
              The GPU test asserts the observed kind of every call of every entry against it, the CPU test ties it to the
              comments of include/msretr.h.
"""
import ctypes as C
import hashlib
import inspect
import os
import re
import time

import numpy as np

import call_sequence_cases as cs

ENQ, SYNC = "enqueue-only", "synchronising"

# ------------------------------------------------------------------------------------------------------------ the delay
# Measured on an MI355X (tests/test_gpu_streams.py prints these with -s): the time from the launch of the sleep to the return
# of the LAST engine method of an entry, over all entries of the four bundles that are enqueue-only throughout, in three runs:
#     longest 1.08 / 0.91 / 1.25 ms (score_docs_union on hyb each time: eight staged copies, then bm25_topk, dense_topk,
#     bm25_score_docs, union_candidates), then rerank_chain on hyb 0.52 / 0.51 / 0.54 ms and merge_topk 0.48 / 0.57 / 0.51 ms;
#     median 0.21 / 0.18 / 0.22 ms.
# MARGIN x 1.25 ms = 5 ms is the least the rule allows (the margin covers host jitter); DELAY_MS is five times that, for a host that shares its cores (a
# delay that runs out shows as a call wrongly seen to synchronise, never as a wrong pass), and a quarter of the cap.  The
# module sleeps about sixty times: 1.5 s of its wall time, plus the 75 ms (HOLD_MS) per entry for which the null stream is held.
LONGEST_ENQUEUE_MS = 1.25
DELAY_MS = 25.0
DELAY_CAP_MS = 100.0
MARGIN = 4                                                    # the delay is at least MARGIN x the longest enqueue time


# ------------------------------------------------------------------------------------------------------------ the table
class Row:
    """method: the DeviceEngine method; c: the C entry points it reaches; kind: ENQ / SYNC as the catalogue calls it (device
    tensors, packed= queries, sets on the device); reason: why it waits (SYNC only); sync_c: the C entry points among `c` that
    wait THEMSELVES (the others only enqueue: the wait is the Python wrapper's); seen: the GPU test observes it (False: the
    kind is from reading the code, no entry run here calls it behind the delay)."""

    def __init__(self, method, c, kind, reason="", sync_c=(), seen=False):
        assert kind in (ENQ, SYNC) and (kind == SYNC) == bool(reason) and set(sync_c) <= set(c), method
        self.method, self.c, self.kind, self.reason, self.sync_c, self.seen = method, tuple(c), kind, reason, tuple(sync_c), seen


_UP = "host upload in the Python wrapper (a blocking copy on the caller's stream)"
_ROWS = [
    # ---- the timed step of bench.py and its neighbours: all enqueue-only
    Row("bm25_topk", ("msr_bm25_topk", "msr_bm25_topk_within"), ENQ, seen=True),       # packed= / DeviceSets; else pack_queries
    Row("bm25_score_docs", ("msr_bm25_score_docs",), ENQ, seen=True),
    Row("union_candidates", ("msr_union_candidates",), ENQ, seen=True),
    Row("dense_topk", ("msr_dense_topk", "msr_dense_topk_within"), ENQ, seen=True),
    Row("dense_begin", ("msr_dense_topk_begin",), ENQ, seen=True),
    Row("dense_end", ("msr_dense_topk_end",), ENQ, seen=True),
    Row("rerank_gather", ("msr_rerank_gather",), ENQ, seen=True),
    Row("rerank_fuse", ("msr_rerank_fuse",), ENQ, seen=True),
    Row("diversify", ("msr_diversify",), ENQ, seen=True),
    Row("merge_topk", ("msr_merge_topk",), ENQ, seen=True),
    Row("rerank", ("msr_rerank",), ENQ),
    Row("merge_gathered", ("msr_merge_topk_payload",), ENQ),
    Row("rerank_gather_blocks", ("msr_rerank_gather_blocks",), ENQ),
    Row("rerank_combine", ("msr_rerank_combine",), ENQ),
    Row("rerank_plan", ("msr_rerank_plan",), ENQ),
    Row("rerank_gather_records", ("msr_rerank_gather_records",), ENQ),
    Row("rerank_scatter", ("msr_rerank_scatter",), ENQ),
    Row("doc_signatures", ("msr_doc_signatures",), ENQ, seen=True),
    Row("bind_signatures", ("msr_bind_signatures",), ENQ, seen=True),                  # launches nothing: keeps the pointer
    Row("collapse_duplicates", ("msr_collapse_scratch_bytes", "msr_collapse_duplicates"), ENQ),
    # ---- host-only reads: launch nothing
    Row("dense_split_max", ("msr_dense_split_max",), ENQ, seen=True),
    Row("dense_path", ("msr_dense_path",), ENQ, seen=True),
    Row("scan_width", ("msr_scan_width",), ENQ, seen=True),
    Row("scan_arith", ("msr_scan_arith",), ENQ),
    Row("batch_width", ("msr_batch_width",), ENQ, seen=True),
    Row("batch_gemm_ok", ("msr_batch_gemm_ok",), ENQ, seen=True),
    Row("row_copy_state", ("msr_row_copy_state",), ENQ),
    Row("row_image_state", ("msr_row_image_state",), ENQ),
    Row("owned_bytes", ("msr_owned_bytes",), ENQ),
    Row("bm25_split", ("msr_debug_bm25_split",), ENQ, seen=True),
    Row("set_timing", ("msr_set_timing",), ENQ),
    Row("has_tokens", (), ENQ), Row("has_vocab", (), ENQ), Row("has_facet", (), ENQ), Row("has_signatures", (), ENQ),
    # ---- synchronising: the C entry point itself waits
    Row("dense_topk_grouped", ("msr_dense_topk_grouped",), SYNC, "reads the group and exclusion offsets on the host",
        ("msr_dense_topk_grouped",), seen=True),
    Row("gather_rows", ("msr_gather_rows",), SYNC, "validates the row numbers on the device", ("msr_gather_rows",), seen=True),
    Row("scratch_dirty", ("msr_debug_scratch_dirty",), SYNC, "the counts come back to the host", ("msr_debug_scratch_dirty",),
        seen=True),
    Row("dense_pass_info", ("msr_dense_pass_info",), SYNC, "a diagnostic: waits for the whole device, then copies the counters",
        ("msr_dense_pass_info",)),
    Row("kernel_time_ms", ("msr_kernel_time_ms",), SYNC, "blocks on the recorded events", ("msr_kernel_time_ms",)),
    Row("rebind", ("msr_unbind", "msr_bind_postings", "msr_bind_tokens", "msr_bind_vocab", "msr_interleave_rows",
                   "msr_bind_chunks", "msr_bind_doc_meta", "msr_enable_bf16"), SYNC,
        "validates the index on the device and reads offsets to the host; the wrapper waits for the device before and after",
        ("msr_bind_postings", "msr_bind_tokens", "msr_bind_vocab", "msr_bind_chunks")),
    Row("bind_facet", ("msr_facet_table", "msr_bind_facet"), SYNC, "validates the table on the device", ("msr_bind_facet",)),
    # ---- synchronising: the C entry point only enqueues, the Python wrapper waits
    Row("debug_select", ("msr_debug_select",), SYNC, "the wrapper copies the select state to the host", seen=True),
    Row("dense_topk_batched", ("msr_dense_topk_bf16", "msr_dense_topk"), SYNC,
        "the wrapper reads which queries overflowed (torch.nonzero) to rerun them", seen=True),
    Row("enable_bf16", ("msr_enable_bf16",), SYNC, "the wrapper waits for the device once the image is built"),
    Row("close", ("msr_destroy",), SYNC, "the wrapper waits for the device before it frees the engine's memory"),
    Row("pack_queries", (), SYNC, _UP, seen=True),
    Row("pack_within", (), SYNC, _UP, seen=True),
    Row("bind_doc_domains", ("msr_bind_doc_domains",), SYNC, _UP),
    Row("term_sets", ("msr_term_sets",), SYNC, _UP),
    Row("phrase_sets", ("msr_term_sets", "msr_phrase_sets", "msr_proximity_sets", "msr_combine_sets"), SYNC, _UP),
    Row("best_windows", ("msr_best_windows",), SYNC, _UP),
    Row("fuzzy_terms", ("msr_fuzzy_scratch_bytes", "msr_fuzzy_terms"), SYNC, "the wrapper copies the candidates to the host"),
    Row("wildcard_terms", ("msr_wildcard_scratch_bytes", "msr_wildcard_terms"), SYNC, "the wrapper copies the matches to the host"),
    Row("facet_counts", ("msr_facet_scratch_bytes", "msr_facet_counts"), SYNC, "the wrapper copies the counts to the host"),
]
TABLE = {r.method: r for r in _ROWS}
assert len(TABLE) == len(_ROWS)

# public names of DeviceEngine that are not calls on a stream
EXCLUDED = {
    "SELECT_STATE": "a numpy record type (the layout of msr_select_state), not a method",
}

# bench.py's timed step: must all be enqueue-only (the issue: otherwise a finding)
HOT_PATH = ("bm25_topk", "dense_topk", "dense_begin", "dense_end", "rerank_gather", "rerank_fuse", "bm25_score_docs",
            "union_candidates", "diversify")

# C entry points without a handle or a stream of the caller's that wait by design (offline builds): in the header, not in the
# table of DeviceEngine methods
OFFLINE_SYNC_C = ("msr_build_postings", "msr_merge_postings", "msr_compact_postings", "msr_debug_exclusive_scan")


# ------------------------------------------------------------------------------------------------------------ the header
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msretr.h")
SAYS_SYNC = re.compile(r"synchronis|waits for the (whole )?device|blocks on", re.I)
SAYS_ENQ = re.compile(r"only enqueue", re.I)


def header_text():
    return open(_HEADER).read()


def header_comment(fn, text=None):
    """The comment of include/msretr.h that documents C function `fn`: the comment block that precedes its prototype (other
    prototypes of the same block may stand in between); where that block has paragraphs of the form "msr_name: ..." or
    "msr_name(args): ...", the paragraph of `fn` alone, plus the block's lines before its first such paragraph."""
    text = header_text() if text is None else text
    m = re.search(r"^(?:int|int64_t|const char\*)\s+%s\(" % re.escape(fn), text, re.M)
    assert m, f"{fn}: no prototype in include/msretr.h"
    end = text.rfind("*/", 0, m.start())
    start = text.rfind("/*", 0, end)
    assert 0 <= start < end, fn
    block = text[start:end]
    para = re.compile(r"^ \*\s{1,6}(msr_\w+)(?:\([^)]*\))?(?:, msr_\w+)*:", re.M)
    marks = [(p.start(), p.group(1)) for p in para.finditer(block)]
    if fn not in [n for _, n in marks]:
        return block
    head = block[:marks[0][0]]
    for i, (pos, name) in enumerate(marks):
        if name == fn:
            return head + block[pos:marks[i + 1][0] if i + 1 < len(marks) else len(block)]


# ------------------------------------------------------------------------------------------------------------ HIP, by ctypes
HIP_STREAM_NON_BLOCKING = 1


def hip_runtime():
    """The HIP runtime torch has loaded (never a second copy of it)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no libamdhip64 is mapped: torch has not initialised HIP")


def stream_flags(hip, handle):
    flags = C.c_uint(0xFFFF)
    rc = hip.hipStreamGetFlags(C.c_void_p(handle), C.byref(flags))
    assert rc == 0, f"hipStreamGetFlags: error {rc}"
    return int(flags.value)


class SideStream:
    """A stream that runs beside the null stream, proven by the control, and the calibrated delay.  .stream: the
    torch.cuda stream; .owned: a hipStream_t this object created (destroyed by close())."""

    TRIES = 4

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.hip = hip_runtime()
        self.owned = []
        self.stream = None
        self.cycles_per_ms = None
        self.block, self.watch = None, None                   # the blocking streams T (hold_null) and U (null_busy)
        self.tried = []
        for _ in range(self.TRIES):
            s = self._non_blocking()
            self.stream = s
            if self.cycles_per_ms is None:
                self._calibrate()
            ok = self.control()
            self.tried.append((s.cuda_stream, ok))
            if ok:
                self.null_control = self.control_null()
                assert all(self.null_control), \
                    f"the window could not be opened: the null stream cannot be held back and watched (idle while the blocking " \
                    f"stream sleeps, the side stream runs meanwhile, a launch on the null stream stays pending): {self.null_control}, " \
                    f"rounds {self.null_rounds}"
                return
        self.stream = None
        raise AssertionError(f"the window could not be opened: on none of {self.TRIES} streams did work behind a sleeping "
                             f"stream stay invisible to the default stream (stream handle, control held): {self.tried}")

    def _non_blocking(self):
        """The next stream of torch's pool if it carries hipStreamNonBlocking; else one created with that flag."""
        torch = self.torch
        s = torch.cuda.Stream(device=self.device)
        if stream_flags(self.hip, s.cuda_stream) & HIP_STREAM_NON_BLOCKING:
            return s
        h = C.c_void_p()
        rc = self.hip.hipStreamCreateWithFlags(C.byref(h), C.c_uint(HIP_STREAM_NON_BLOCKING))
        assert rc == 0, f"hipStreamCreateWithFlags: error {rc}"
        self.owned.append(h)
        s = torch.cuda.ExternalStream(h.value, device=self.device)
        assert stream_flags(self.hip, s.cuda_stream) & HIP_STREAM_NON_BLOCKING
        return s

    def _calibrate(self):
        """Cycles of torch.cuda._sleep per millisecond, between two events; the count grows until the sleep lasts >= 2 ms (the
        unit of the spin kernel's counter is not assumed)."""
        torch, n = self.torch, 100_000
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(1000)                           # (the first launch of the kernel: not timed)
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(self.stream):
                a.record()
                torch.cuda._sleep(n)
                b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0 or n >= 1 << 40:
                break
            n *= 8
        assert 2.0 <= ms <= DELAY_CAP_MS, f"torch.cuda._sleep({n}) took {ms} ms"
        self.cycles_per_ms = n / ms

    def sleep(self, ms=DELAY_MS):
        """The delay, on the CURRENT stream."""
        assert 0 < ms <= DELAY_CAP_MS
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def control(self, ms=DELAY_MS):
        """While S sleeps, a write enqueued on S behind the sleep must not be seen by an ordinary default-stream read."""
        torch = self.torch
        marker = torch.zeros((64,), dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(self.stream):
            self.sleep(ms)
            marker.fill_(1)
        early = marker.cpu()                                  # default stream; returns when ITS copy is done
        self.stream.synchronize()
        late = marker.cpu()
        assert int(late.sum()) == 64, "the write behind the sleep never landed"
        return int(early.sum()) == 0

    # -- the null stream held back: ANY launch that strays to it is seen, whether or not it changes a result
    # A stray launch whose product no result depends on (the BM25 plan kernel: the order of the work items and the window
    # anchors, both documented as "the result never depends on it") gives the right bytes even behind the delay.  So while an
    # entry runs, a BLOCKING stream T sleeps: the null stream waits for blocking streams, the side stream (non-blocking) does
    # not.  Work launched on the null stream is then still pending when the entry has read its outputs from the side stream
    # -- null_busy() says so -- and the null stream is empty if nothing strayed.
    HOLD_MS = 3 * DELAY_MS

    def hold_null(self, ms=None):
        """A sleep on the blocking stream T -> the event behind it (pending: the null stream is still held)."""
        torch = self.torch
        if self.block is None:
            self.block = self._blocking()
        ev = torch.cuda.Event()
        with torch.cuda.stream(self.block):
            self.sleep(self.HOLD_MS if ms is None else ms)
            ev.record()
        return ev

    def null_busy(self, wait_ms=5.0):
        """True while work enqueued on the null stream has not completed.  hipStreamQuery(null) cannot tell: it says "not
        ready" for the blocking stream's sleep alone.  But a blocking stream waits for the null stream's pending work and not
        for another blocking stream's: an event recorded on a SECOND blocking stream U completes at once when the null stream
        is empty and stays behind the held null stream's work otherwise (both shown by control_null)."""
        torch = self.torch
        if self.watch is None:
            self.watch = self._blocking()
        ev = torch.cuda.Event()
        ev.record(self.watch)
        t0 = time.perf_counter()
        while 1e3 * (time.perf_counter() - t0) < wait_ms:
            if ev.query():
                return False
        return True

    def _blocking(self):
        h = C.c_void_p()
        rc = self.hip.hipStreamCreateWithFlags(C.byref(h), C.c_uint(0))
        assert rc == 0, f"hipStreamCreateWithFlags: error {rc}"
        self.owned.append(h)
        s = self.torch.cuda.ExternalStream(h.value, device=self.device)
        assert stream_flags(self.hip, h.value) & HIP_STREAM_NON_BLOCKING == 0
        return s

    def release_null(self):
        self.block.synchronize()
        self.torch.cuda.synchronize(self.device)
        assert not self.null_busy()

    def control_null(self):
        """The detector's own control: with T asleep the null stream is idle; one kernel launched on it stays pending; the side
        stream runs meanwhile; with T awake again the null stream drains.  -> (idle, side_ran, seen).  A round in which T woke
        before the last look (the host was held up for longer than HOLD_MS) decides nothing and is taken again.  A round that
        decides against the streams (T or U on a hardware queue with another stream of the control: one of them then waits
        for the other's sleep) takes two new blocking streams: choosing streams, as for the side stream.  TRIES rounds at the
        most; self.null_rounds keeps (ms from the hold to the last look, T still asleep then, the three findings)."""
        torch = self.torch
        if self.block is None:
            self.block = self._blocking()
        if self.watch is None:
            self.watch = self._blocking()
        x = torch.zeros((64,), dtype=torch.int32, device=self.device)
        y = torch.zeros((64,), dtype=torch.int32, device=self.device)
        self.null_rounds = []
        for _ in range(self.TRIES):
            x.zero_()
            y.zero_()
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            held = self.hold_null()
            idle = not self.null_busy()
            with torch.cuda.stream(self.stream):
                y.fill_(1)
                side_ran = int(y.cpu().sum()) == 64           # (the side stream does not wait for T: T is asleep below)
            x.fill_(1)                                        # the default stream IS the null stream
            seen = self.null_busy()
            asleep = not held.query()
            self.null_rounds.append((round(1e3 * (time.perf_counter() - t0), 2), asleep, (idle, side_ran, seen)))
            self.release_null()
            assert int(x.cpu().sum()) == 64
            if asleep and idle and side_ran and seen:
                break
            if asleep:
                self.block, self.watch = self._blocking(), self._blocking()
        assert asleep, f"the host was held up in every round of the control: {self.null_rounds}"
        return idle, side_ran, seen

    def close(self):
        self.torch.cuda.synchronize(self.device)
        for h in self.owned:
            self.hip.hipStreamDestroy(h)
        self.owned = []


# ------------------------------------------------------------------------------------------------------------ the stage
def _digest(*parts):
    h = hashlib.blake2b(digest_size=12)
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(str((p.dtype, p.shape)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def _rot(a, axis=0):
    return np.ascontiguousarray(np.roll(a, 1, axis=axis))


def decoy_of(bundle, key, a):
    """The decoy of input `key`: the real input rotated by one query -- the same values, every one valid where it stands,
    another answer.  Two inputs need their own rule: the shard lists of merge_topk are [shard, query, k] (rotating the shards
    gives the same merge), and the 55 rows of grouped_global_record_overflow are one row repeated (its decoy: another row)."""
    if isinstance(key, tuple) and key[0] == "merge":
        return _rot(a, 1 if a.ndim >= 2 else 0)
    if key == ("q", "grouped50"):
        return np.ascontiguousarray(np.repeat(bundle.inp.rows(1, shift=9)[1], a.shape[0], axis=0), np.float32)
    return _rot(a, 0)


class Stage:
    """REAL, DECOY and LIVE copies of every device input of one bundle."""

    def __init__(self, torch):
        self.torch = torch
        self.bundle = None
        self.real, self.decoy, self.live = {}, {}, {}
        self.used = set()
        self.sealed = False                                   # True behind the delay: a new input would need a host upload
        self._packs, self._sets = {}, {}

    def adopt(self, key, a):
        assert key is not None, "a staged input needs a key"
        if key not in self.live:
            assert not self.sealed, f"input {key} first appears behind the delay (the decoy run did not use it)"
            dev = self.bundle.eng.device
            d = decoy_of(self.bundle, key, a)
            assert d.shape == a.shape and d.dtype == a.dtype, key
            self.real[key] = self.torch.from_numpy(a).to(dev)
            self.decoy[key] = self.torch.from_numpy(d).to(dev)
            self.live[key] = self.decoy[key].clone()
        self.used.add(key)
        return self.live[key]

    def touch(self, key):
        for k in self.live:
            if k == key or (isinstance(k, tuple) and isinstance(key, tuple) and k[:len(key)] == key):
                self.used.add(k)

    def load(self, which, keys=None):
        """LIVE <- DECOY / REAL by device-to-device copies on the current stream (nothing blocks the host)."""
        src = self.decoy if which == "decoy" else self.real
        for k in (self.live if keys is None else keys):
            self.live[k].copy_(src[k], non_blocking=True)

    # -- what an entry hands to an engine METHOD from the host
    def array(self, method, arg, a):
        return self.adopt(("arg", _digest(a)), np.ascontiguousarray(a))

    def packed(self, eng, term_lists):
        """bm25_topk's / bm25_score_docs' packed= form of the term lists (decoy: the lists rotated by one query)."""
        lists = [list(map(int, t)) for t in term_lists]
        key = ("pack", _digest(lists))
        if key not in self._packs:
            assert not self.sealed, "term lists first appear behind the delay"
            real, decoy = eng.pack_queries(lists), eng.pack_queries(lists[-1:] + lists[:-1])
            for i in range(3):
                assert real[i].shape == decoy[i].shape
                k = key + (i,)
                self.real[k], self.decoy[k], self.live[k] = real[i], decoy[i], decoy[i].clone()
            self._packs[key] = real[3]
        for i in range(3):
            self.used.add(key + (i,))
        return self.live[key + (0,)], self.live[key + (1,)], self.live[key + (2,)], self._packs[key]

    def within(self, eng, within, n_queries):
        """A list of DocSets as sets on the device (docset.DeviceSets), q_set staged (decoy: rotated by one query)."""
        from msretr.docset import DeviceSets
        if within is None or isinstance(within, DeviceSets):
            return within
        sets = list(within) if isinstance(within, (list, tuple)) else [within] * n_queries
        key = ("within", id(eng.index), tuple(id(s) for s in sets))
        if key not in self._sets:
            assert not self.sealed, "document sets first appear behind the delay"
            bits, q_set, n_sets, stride = eng.pack_within(sets, n_queries)
            self.real[key] = q_set
            self.decoy[key] = self.torch.roll(q_set, 1)
            self.live[key] = self.decoy[key].clone()
            self._sets[key] = (DeviceSets(eng.index, bits, self.live[key], n_sets, stride), sets)     # (keeps the DocSets alive)
        self.used.add(key)
        return self._sets[key][0]


# the arguments of engine methods that the stage turns into device inputs: (host arrays, term lists, document sets)
STAGED_ARGS = {
    "bm25_topk": ((), "term_lists", "within"),
    "bm25_score_docs": (("doc", "doc_n"), "term_lists", None),
    "union_candidates": (("dense_doc", "dense_bm25", "dense_n"), None, None),
    "dense_topk": (("qvec",), None, "within"),
    "dense_begin": (("qvec",), None, None),
    "dense_topk_batched": (("qvec",), None, None),
    "dense_topk_grouped": (("qvec",), None, None),
    "rerank_gather": (("qvec", "cand_doc_global", "cand_n"), None, None),
    "rerank_fuse": (("cand_doc_global", "cand_bm25", "cand_n"), None, None),
}


class Observed:
    """A DeviceEngine seen through the stage: host arguments become staged device inputs, and every public method call notes
    whether the event behind the delay was pending when it was entered and when it returned."""

    def __init__(self, eng, stage):
        object.__setattr__(self, "_eng", eng)
        object.__setattr__(self, "_stage", stage)
        object.__setattr__(self, "event", None)
        object.__setattr__(self, "seen", [])                  # (method, pending at entry, pending at return, host time of return)
        object.__setattr__(self, "calls", 0)

    def __setattr__(self, name, value):
        if name in ("event", "seen", "calls"):
            object.__setattr__(self, name, value)
        else:
            setattr(self._eng, name, value)

    def __getattr__(self, name):
        v = getattr(self._eng, name)
        if name.startswith("_") or not inspect.ismethod(v):
            return v

        def call(*args, **kw):
            eng, stage = self._eng, self._stage
            if name in STAGED_ARGS:
                arrays, lists, sets = STAGED_ARGS[name]
                ba = inspect.signature(v).bind(*args, **kw)
                a = ba.arguments
                for n in arrays:
                    if isinstance(a.get(n), np.ndarray):
                        a[n] = stage.array(name, n, a[n])
                if lists and a.get(lists) is not None and a.get("packed") is None:
                    a["packed"], a[lists] = stage.packed(eng, a[lists]), None
                if sets and a.get(sets) is not None:
                    a[sets] = stage.within(eng, a[sets], a["packed"][3] if "packed" in a and a["packed"] else
                                           int(a["qvec"].shape[0]))
                args, kw = ba.args, ba.kwargs
            ev = self.event
            before = ev is not None and not ev.query()
            object.__setattr__(self, "calls", self.calls + 1)
            out = v(*args, **kw)
            after = ev is not None and not ev.query()
            self.seen.append((name, before, after, time.perf_counter()))
            return out
        return call


class StagedBundle(cs.Bundle):
    """A catalogue bundle whose engine lives on the side stream and whose inputs are staged.  Built inside
    `with torch.cuda.stream(S)`: creation, every bind, enable_bf16 and the retriever."""

    def __init__(self, name, torch):
        stage = Stage(torch)
        stage.bundle = self
        super().__init__(name, stage=stage)
        self.real_eng = self.eng
        self.eng = Observed(self.real_eng, stage)

    def dev(self, key, make):
        out = super().dev(key, make)
        self.stage.touch(key)
        return out

    def close(self):
        self.real_eng.close()


# ------------------------------------------------------------------------------------------------------------ the entries
def _split_with_bound(b):
    """dense_begin / dense_end with a bound: one shard, so the bound is the shard's own part (the minimum over one shard)."""
    _, q = b.inp.rows(100)
    part = b.eng.dense_begin(b.qdev(("rows", 100), q), k=cs.K_DENSE)
    out = cs._host(part, *b.eng.dense_end(100, k=cs.K_DENSE, bound=part))
    return cs._named(("part", "doc", "score", "chunk", "n"), out), dict(dense_path=b.eng.dense_path())


def _chk_split_with_bound(b, out, rep):
    """K_DENSE documents of the shard reach the bound exactly, so nothing of the top k is dropped: the lists are those of the
    call without a bound, bit for bit (include/msretr.h: "the merged list is the unsharded one")."""
    assert rep["dense_path"] == 128 and (out["n"] == cs.K_DENSE).all()
    clean = b.clean["dense_begin_end"]
    assert all(out[a].tobytes() == clean[a].tobytes() for a in clean), "dense_end with its own bound differs from dense_end without"


SPLIT_WITH_BOUND = cs.Entry("split_begin_end_with_bound", "dirtier", cs.DENSE, _split_with_bound,
                            ("dense_begin", "dense_end", "dense_path"), check=_chk_split_with_bound, group="split")

# the dirtiers that leave through a fallback with FURTHER LAUNCHES (a refusal launches nothing and need not run here)
FALLBACK_DIRTIERS = ("dense_zero_query_in_100", "dense_zero_query_in_200", "dense_twin_group_above_pair_cap",
                     "bf16_sel_cap_overflow_100", "bf16_sel_cap_overflow_200", "grouped_global_record_overflow")

# a probe whose inputs cannot be staged: it takes host lists and uploads them inside the call
HOST_INPUT_PROBES = {
    "final_lists_hybrid": "goes through Retriever.final_lists, which takes host term lists and vectors and uploads them itself: "
                          "it runs behind the delay and is checked against the oracle and the default stream, without a decoy",
}


def entries_on_stream(bundle_name):
    """The entries test_gpu_streams.py runs for a bundle, in order: its probes (select_f32 first), then the fallback
    dirtiers of the bundle and the split with a bound."""
    out = cs.entries_for(bundle_name, "probe")
    out += [cs.by_name(n) for n in FALLBACK_DIRTIERS if bundle_name in cs.by_name(n).bundles]
    if bundle_name in SPLIT_WITH_BOUND.bundles:
        out.append(SPLIT_WITH_BOUND)
    return out


def run_on_stream(b, entry, side):
    """The staged run of one entry on the CURRENT stream (the side stream) ->
    (outputs, report, decoy outputs, [(method, kind observed)], ms from the sleep's launch to the last method's return, the
    staged inputs the entry read, work was pending on the held null stream when the entry had read its outputs, the null
    stream was still held then)."""
    torch, stage, eng = b.torch, b.stage, b.eng
    # 1: decoys in every live input, the entry once, synchronised
    eng.event, stage.sealed = None, False
    stage.load("decoy")
    torch.cuda.current_stream().synchronize()
    stage.used = set()
    decoy_out, _ = entry.run(b)
    torch.cuda.current_stream().synchronize()
    used = sorted(stage.used, key=repr)
    # 2: the null stream held back; the delay, the event, the real inputs behind them
    assert not side.null_busy()
    held = side.hold_null()
    ev = torch.cuda.Event()
    t0 = time.perf_counter()
    side.sleep()
    ev.record()
    stage.load("real", used)
    # 3, 4: the entry; Observed notes the event at every return
    eng.event, eng.seen, stage.sealed = ev, [], True
    try:
        out, rep = entry.run(b)                               # 5: the entry reads its outputs itself (on this stream)
        stray, conclusive = side.null_busy(), not held.query()
    finally:
        seen, eng.event, stage.sealed = eng.seen, None, False
        side.release_null()
    kinds = [(m, ENQ if after else SYNC) for m, before, after, _ in seen if before]
    t_last = max([t for _, before, _, t in seen if before], default=t0)
    return out, rep, decoy_out, kinds, 1e3 * (t_last - t0), used, stray, conclusive
