"""Match modes on the host (match.py, DESIGN K19), without a GPU: the need table, a query's slots, the option's check, that the
text syntax does not see the option, that the header of the new call and its binding agree while include/msretr.h is as it
was, the numpy oracle on hand-written rows, and the call's argument checks under the host sanitizers."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from match_ref import group_mask, match_mask, match_words, pack
from msretr import _abi, match
from msretr.query import Conditions, SearchOptions, parse_queries
from msretr.text import simple_tokenize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modern-search-engines-project_amd", "csrc")


# ------------------------------------------------------------------------------------------------ need
@pytest.mark.parametrize("value, G, want", [
    ("any", 3, None), (None, 3, None), ("all", 3, 3), ("all", 1, 1), ("all", 64, 64),
    (2, 3, 2), (1, 3, 1), (3, 3, 3), (np.int64(2), 3, 2),
    (-1, 3, 2), (-2, 3, 1),
    ("75%", 4, 3), ("75%", 3, 2), ("75%", 8, 6), ("100%", 5, 5), ("50%", 3, 1),
    ("-25%", 4, 3), ("-25%", 8, 6), ("-25%", 3, 3), ("-100%", 4, 1),
    # the clamps: never below 1, never above the number of slots
    (5, 3, 3), (100, 1, 1), (-3, 3, 1), (-7, 3, 1), ("10%", 3, 1), ("1%", 64, 1), ("-99%", 3, 1),
    # a query without slots: nothing to require
    ("all", 0, None), (2, 0, None), ("75%", 0, None),
])
def test_need_table(value, G, want):
    assert match.need(value, G) == want


@pytest.mark.parametrize("value", [True, False, 0, np.int32(0), "0%", "-0%", 0.5, 2.0, "", "ALL", "some", "75", "75 %", "7.5%",
                                   "101%", "1000%", "%", "+75%", "--5%", [2], ("all",), b"all"])
def test_need_refuses(value):
    with pytest.raises(ValueError, match="match must be"):
        match.need(value, 3)
    with pytest.raises(ValueError):
        match.check_value(value)
    with pytest.raises(ValueError):                          # also where it would not matter: a query without slots
        match.need(value, 0)


# ------------------------------------------------------------------------------------------------ slots
def _ix(idf):
    return SimpleNamespace(n_terms=len(idf), idf=np.asarray(idf, np.float32))


def test_slots():
    ix = _ix([-0.7, 1.0, 2.0, 0.5, 0.0, 1.5])                # term 0: the city (idf < 0); term 4: idf == 0
    assert match.slots(ix, [1, 2, 3]) == [[1], [2], [3]]
    assert match.slots(ix, [3, 1, 3, 1, 2, 3]) == [[3], [1], [2]]                    # duplicates: first occurrence first
    assert match.slots(ix, [1, 0, 2]) == [[1], [2]]                                  # the city term is no slot
    assert match.slots(ix, [1, 4]) == [[1]]                                          # idf == 0 neither
    assert match.slots(ix, [0]) == [[0]] and match.slots(ix, [4, 0, 4]) == [[4], [0]]    # the fallback: all are kept
    assert match.slots(ix, [1, -1, 2]) == [[1], [2], [-1]]                           # a word the vocabulary lacks: its own slot
    assert match.slots(ix, [-1, 6, 99, -5]) == [[-1]] * 4                            # ... each of them, whatever the id
    assert match.slots(ix, [-1, 0]) == [[0], [-1]]                                   # (the fallback looks at the known words)
    assert match.slots(ix, []) == [] and match.slots(ix, [], []) == []
    # a pattern's expansions are ONE slot, behind the words; an id twice in it counts once; an empty expansion is an empty slot
    assert match.slots(ix, [1, 0], [[2, 3, 2], []]) == [[1], [2, 3], []]
    assert match.slots(ix, [], [[5, 1]]) == [[5, 1]]
    assert match.slots(ix, [1], [[1, 0]]) == [[1], [1, 0]]                           # a term in two slots fills both
    assert match.slots(ix, np.asarray([2, 2, 1], np.int32)) == [[2], [1]]
    assert "`tübingen` is therefore not required either" in " ".join(match.slots.__doc__.split())
    # the need of such slots
    assert match.need("all", len(match.slots(ix, [1, 0, 2]))) == 2
    assert match.need("all", len(match.slots(ix, [1, -1, 2]))) == 3
    # names for the result
    names = match.slot_names([[1], [2, 3], [-1], [], [-1]], lambda t: f"t{t}", ["typo"])
    assert names == [["t1"], ["t2", "t3"], ["typo"], [], [None]]


# ------------------------------------------------------------------------------------------------ the option
def test_search_options_check():
    for ok in ("any", None, "all", 1, 2, -1, 64, 1000, "75%", "-25%", "100%", np.int64(3)):
        SearchOptions(match=ok).check()
    assert SearchOptions().match == "any" and not SearchOptions().match_on and not SearchOptions(match=None).match_on
    assert SearchOptions(match="all").match_on and SearchOptions(match=2).match_on
    for bad in (True, False, 0, "0%", 1.5, "most", "75", "200%"):
        with pytest.raises(ValueError, match="match must be"):
            SearchOptions(match=bad).check()
    with pytest.raises(ValueError):
        SearchOptions(match="0%").check(patterns=True, int_types=int)


def test_parse_queries_does_not_see_the_option():
    texts = ['mensa +morgenstelle -"alte aula" öffnungszeiten', 'bibliothek* "wilhelm strasse"~2 tübingen', "plain words"]
    explicit = Conditions(must=[["a"], [], []], must_not=[[], ["b"], []])
    for kw in (dict(), dict(operators=True), dict(operators=True, phrases=True, wildcards=True),
               dict(proximity=True, wildcards=True)):
        want = parse_queries(texts, simple_tokenize, SearchOptions(**kw), explicit, None)
        for value in ("all", 2, "75%"):
            assert parse_queries(texts, simple_tokenize, SearchOptions(match=value, **kw), explicit, None) == want


def test_sharded_engine_refuses_the_option():
    from msretr.distributed import ShardedEngine
    sharded = ShardedEngine.__new__(ShardedEngine)           # (the refusal comes before anything of the engine is read)
    for value in ("all", 2, "75%"):
        with pytest.raises(ValueError, match="match= is not available on a sharded engine"):
            sharded.search([[1]], None, match=value)


# ------------------------------------------------------------------------------------------------ header and binding
def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_and_binding_agree():
    hdr = _read("include", "msretr_match.h")
    m = re.search(r"^int msr_match_sets\(([^;]*)\);", hdr, re.M | re.S)
    assert m, "no prototype of msr_match_sets in include/msretr_match.h"
    args = [a.strip() for a in m.group(1).split(",")]
    res, bound = _abi._SIGNATURES["msr_match_sets"]
    assert len(args) == len(bound) == 13 and res is _abi.C.c_int
    assert args[0] == "msr_engine* e" and args[-1] == "void* stream"
    for a, b in zip(args, bound):                            # pointers, 32-bit counts and 64-bit strides where the header has them
        want = _abi._P if "*" in a else _abi.C.c_int64 if a.startswith("int64_t") else _abi.C.c_int32
        assert b is want, (a, b)
    assert int(re.search(r"#define MSR_MATCH_MAX_GROUPS (\d+)", hdr).group(1)) == _abi.MSR_MATCH_MAX_GROUPS == 64
    assert _abi.MSR_MATCH_MAX_GROUPS == _abi.MSR_MAX_QUERY_TERMS == match.MSR_MATCH_MAX_GROUPS
    assert '#include "msretr.h"' in hdr and "only enqueues" in hdr and "MSR_ERR_NOT_BOUND" in hdr
    # the main header is what it was: no new prototype, the same version; the new call is not one of ITS exports
    main = _read("include", "msretr.h")
    assert "msr_match_sets" not in main and "msretr_match" not in main
    assert int(re.search(r"#define MSR_ABI_VERSION (\d+)", main).group(1)) == _abi.MSR_ABI_VERSION == 16
    assert "msr_match_sets" not in _abi.EXPORTS and _abi.MATCH_EXPORTS == ("msr_match_sets",)
    assert set(_abi.EXPORTS) | set(_abi.MATCH_EXPORTS) == set(_abi._SIGNATURES)
    assert hasattr(_abi.load(), "msr_match_sets")
    # the engine gained no public name for it
    from msretr.engine import DeviceEngine
    assert not [n for n in vars(DeviceEngine) if "match" in n and not n.startswith("_")]
    from msretr.build import UNITS
    assert "msr_match.hip" in UNITS and os.path.exists(os.path.join(CSRC, "msr_match.hip"))


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_on_hand_written_rows():
    # 40 documents (two words, the second partial), 4 terms: A = {0, 1, 2, 33}, B = {1, 2, 39}, C = {2, 33}, D = {} (empty)
    lists = [[0, 1, 2, 33], [1, 2, 39], [2, 33], []]
    z = {"term_off": np.cumsum([0] + [len(l) for l in lists]), "post_doc": np.concatenate([np.asarray(l, np.int64) for l in lists]),
         "n_docs": 40}
    A, B, Cc, D = range(4)
    docs = lambda mask: np.nonzero(mask)[0].tolist()
    assert docs(group_mask(z, [A, B])) == [0, 1, 2, 33, 39] and docs(group_mask(z, [D, -1, 4, 99])) == []
    # row 1: at least 2 of {A}, {B}, {C}: counts 0:1 1:2 2:3 33:2 39:1
    assert docs(match_mask(z, [[A], [B], [Cc]], 2)) == [1, 2, 33]
    assert match_words(z, [[A], [B], [Cc]], 2).tolist() == [0b110, 0b10]
    # row 2: all of {A, B} (one group, a document in both counts once), {C}, inside a base without document 2
    base = np.ones(40, bool)
    base[2] = False
    assert docs(match_mask(z, [[A, B], [Cc]], 2, base)) == [33] and docs(match_mask(z, [[A, B], [Cc]], 2)) == [2, 33]
    # row 3: the same term in two groups fills both; an unknown word is a slot that nobody fills
    assert docs(match_mask(z, [[B], [B], [-1]], 2)) == [1, 2, 39] and docs(match_mask(z, [[B], [B], [-1]], 3)) == []
    # the conventions
    assert docs(match_mask(z, [[A]], 0, base)) == docs(base) and docs(match_mask(z, [], -3)) == list(range(40))
    assert docs(match_mask(z, [[A]], 2)) == [] and docs(match_mask(z, [], 1)) == []
    assert docs(match_mask(z, [[A]] * 64, 64)) == [0, 1, 2, 33] and docs(match_mask(z, [[A]] * 65, 1)) == []
    assert pack(np.ones(40, bool)).tolist() == [0xFFFFFFFF, 0xFF] and pack(np.zeros(0, bool)).tolist() == []


# ------------------------------------------------------------------------------------------------ the argument checks
def test_argument_checks_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "match_args_check")
    # (the sanitizer runtime linked statically: the program starts the same whatever else the environment preloads)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-I" + CSRC, os.path.join(ROOT, "tests", "match_args_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match args ok" in r.stdout
