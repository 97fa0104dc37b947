"""The table of what synchronises (tests/stream_cases.py), checked without a GPU against the engine's methods and against the
comments of include/msretr.h.  That the table equals what the GPU does is test_gpu_streams.py's part; here: every public
DeviceEngine method has a row, every C entry point a row calls synchronising says so in its OWN comment of the header, and no
comment that says "only enqueues" stands over a function of the synchronising column."""
import re

import numpy as np

import call_sequence_cases as cs
import stream_cases as sx


def test_every_public_method_of_the_engine_has_a_row():
    from msretr.engine import DeviceEngine
    public = {n for n in vars(DeviceEngine) if not n.startswith("_")}       # methods, properties and class attributes
    assert set(sx.TABLE) <= public and set(sx.EXCLUDED) <= public, sorted((set(sx.TABLE) | set(sx.EXCLUDED)) - public)
    assert not set(sx.TABLE) & set(sx.EXCLUDED)
    assert all(isinstance(r, str) and len(r) > 20 for r in sx.EXCLUDED.values())
    missing = public - set(sx.TABLE) - set(sx.EXCLUDED)
    assert not missing, f"DeviceEngine names without a row in stream_cases.TABLE and not excluded with a reason: {sorted(missing)}"
    for r in sx.TABLE.values():
        assert r.kind in (sx.ENQ, sx.SYNC) and (r.kind == sx.SYNC) == (len(r.reason) > 20), r.method
        assert r.kind == sx.SYNC or not r.sync_c, r.method    # a method over a waiting C call waits
    assert set(sx.HOT_PATH) <= set(sx.TABLE) and all(sx.TABLE[m].kind == sx.ENQ and sx.TABLE[m].seen for m in sx.HOT_PATH)
    assert set(sx.STAGED_ARGS) <= set(sx.TABLE)


def test_the_rows_name_c_entry_points_the_abi_has():
    from msretr import _abi
    text = sx.header_text()
    for r in sx.TABLE.values():
        for fn in r.c:
            assert re.search(r"^(?:int|int64_t)\s+%s\(" % fn, text, re.M), (r.method, fn)
            assert fn in _abi._SIGNATURES, (r.method, fn)
    # every entry point of the ABI that takes a stream is reached by a row, or is one of the handle-less offline / test calls
    with_stream = {m.group(1) for m in re.finditer(r"^int\s+(msr_\w+)\((?:[^;]*?)void\* stream\);", text, re.M | re.S)}
    reached = {fn for r in sx.TABLE.values() for fn in r.c}
    other = set(sx.OFFLINE_SYNC_C) | {"msr_debug_count_nonzero"}
    assert with_stream - reached - other == set(), sorted(with_stream - reached - other)


def test_the_header_says_what_the_table_says():
    text = sx.header_text()
    sync_c = {fn for r in sx.TABLE.values() for fn in r.sync_c} | set(sx.OFFLINE_SYNC_C)
    for fn in sorted(sync_c):
        c = sx.header_comment(fn, text)
        assert sx.SAYS_SYNC.search(c), f"{fn} waits for the stream (stream_cases.TABLE) but its comment in include/msretr.h does not say so"
        assert not sx.SAYS_ENQ.search(c), f"{fn}: its comment says 'only enqueues', the table says it waits"
    # and the other way round: a function whose own comment says "only enqueues" is in no synchronising column
    protos = re.findall(r"^int\s+(msr_\w+)\(", text, re.M)
    says_enq = {fn for fn in protos if sx.SAYS_ENQ.search(sx.header_comment(fn, text))}
    assert len(says_enq) >= 10 and not says_enq & sync_c, sorted(says_enq & sync_c)
    # the convention itself: no "nothing synchronises", the rule, and the calls that wait named in it
    head = text[:text.index("#ifndef MSRETR_H")]
    assert "nothing synchronises" not in head and "only enqueue" in head
    for fn in sorted({fn for r in sx.TABLE.values() for fn in r.sync_c}):
        assert fn in head, f"{fn} waits but the convention at the top of include/msretr.h does not name it"
    assert re.search(r"DEVICE-WIDE WAIT", sx.header_comment("msr_dense_pass_info", text))
    assert re.search(r"waits for them", sx.header_comment("msr_create", text))


def test_the_entries_and_their_decoys():
    assert [e.name for e in sx.entries_on_stream("lex")][0] == "select_f32"
    for bn in cs.ALL:
        names = [e.name for e in sx.entries_on_stream(bn)]
        assert names[0] == "select_f32" and len(names) == len(set(names))
        assert {p.name for p in cs.entries_for(bn, "probe")} <= set(names)
    ran = {e.name for bn in cs.ALL for e in sx.entries_on_stream(bn)}
    assert set(sx.FALLBACK_DIRTIERS) | {sx.SPLIT_WITH_BOUND.name} <= ran
    assert set(sx.HOST_INPUT_PROBES) <= {p.name for p in cs.PROBES}
    # the decoys: valid inputs of the same shapes that are not the inputs
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    assert sx.decoy_of(None, ("q", "x"), a).tolist() == np.roll(a, 1, axis=0).tolist()
    d, s, n = cs.merge_lists_input()
    for i, x in enumerate((d, s, n)):
        y = sx.decoy_of(None, ("merge", i), x)
        assert y.shape == x.shape and (y.tobytes() != x.tobytes() or i == 2)      # (the counts are all k)
        assert (y[:, 1] == x[:, 0]).all()                     # the QUERIES are rotated, not the shards
    assert 0 < sx.MARGIN * sx.LONGEST_ENQUEUE_MS <= sx.DELAY_MS <= sx.SideStream.HOLD_MS <= sx.DELAY_CAP_MS == 100.0
