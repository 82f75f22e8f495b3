"""CPU: the surface of the device lookup (include/mox.h mox_lookup_words, the
Python mirror, dist.sum_lookups) and the case tables of test_gpu_lookup.py
(lookup_cases.py).  No GPU code runs here."""
import ctypes
import os
import re

import numpy as np
import pytest

import join_cases as J
import lookup_cases as C
import mox
from mox import dist as mdist
from conftest import ROOT
from srcpins import _read, code_only, op_objects


def test_header_declares_the_lookup():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    assert "#define MOX_LOOKUP_MAX (1u << 20)" in src and "#define MOX_LOOKUP_NONE (~0ull)" in src
    assert ("int mox_lookup_words(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, "
            "uint64_t* counts, uint64_t* index, mox_lookup_info* info);") in src
    m = re.search(r"typedef struct mox_lookup_info \{(.*?)\} mox_lookup_info;", src)
    assert m, "mox_lookup_info"
    assert re.findall(r"uint64_t ([a-z_]+)(?:\[(\d+)\])?;", m.group(1)) == [
        ("queries", ""), ("distinct", ""), ("found", ""), ("tag_mismatch", ""), ("reserved", "4")]
    assert ctypes.sizeof(mox.LookupInfo) == 64
    assert [f for f, _ in mox.LookupInfo._fields_] == ["queries", "distinct", "found", "tag_mismatch", "reserved"]
    assert mox.LOOKUP_MAX == 1 << 20 == C.LOOKUP_MAX and mox.LOOKUP_NONE == (1 << 64) - 1 == C.NONE
    # the contract is written down next to the declaration
    doc = raw.split("looking words up in the device-resident result")[1].split("mox_get_stats")[0]
    for phrase in ("lowercase", "verbatim", "MOX_ESTATE", "MOX_EINVAL", "untouched", "MOX_LOOKUP_GRID", "mox_top_words"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_the_lookup(path):
    assert hasattr(ctypes.CDLL(path), "mox_lookup_words")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_lookup_words
    U64P = ctypes.POINTER(ctypes.c_uint64)
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_void_p, U64P, ctypes.c_uint64, U64P, U64P,
                                ctypes.POINTER(mox.LookupInfo)]


def test_null_engine_is_einval_and_leaves_the_outputs():
    L = mox.lib()
    offs = (ctypes.c_uint64 * 3)(0, 1, 2)
    counts = (ctypes.c_uint64 * 2)(7, 8)
    index = (ctypes.c_uint64 * 2)(9, 10)
    info = mox.LookupInfo(queries=5, distinct=6, found=7, tag_mismatch=8)
    assert L.mox_lookup_words(None, b"ab", offs, 2, counts, index, ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    assert list(counts) == [7, 8] and list(index) == [9, 10]
    assert (info.queries, info.distinct, info.found, info.tag_mismatch) == (5, 6, 7, 8)


def test_python_surface():
    assert callable(mox.Engine.lookup) and callable(mox.Engine.lookup_packed) and callable(mdist.sum_lookups)


def test_constants_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_lookup.hip")
    ws = _read("map-oxidize_amd", "csrc", "mox_wordset.h")  # the geometry is the word set's, shared with the join
    t = int(re.search(r"^constexpr int WS_T = (\d+);", ws, re.M).group(1))
    per = int(re.search(r"^constexpr int WS_PER = (\d+);", ws, re.M).group(1))
    assert re.search(r"^constexpr uint32_t WS_TILE = WS_T \* WS_PER;", ws, re.M)
    assert t * per == C.TILE == J.TILE and t % 64 == 0
    assert int(re.search(r"^constexpr uint32_t WS_LANE_MAX = (\d+);", ws, re.M).group(1)) == C.LANE_MAX
    policy = re.search(r"^struct LkWords \{(.*?)^\};", src, re.M | re.S).group(1)  # the slot split is the lookup's policy
    assert int(re.search(r"^  static constexpr int IDX_BITS = (\d+);", policy, re.M).group(1)) == C.IDX_BITS
    assert int(re.search(r"^  static constexpr int TAG_BITS = (\d+);", policy, re.M).group(1)) == C.TAG_BITS
    assert C.IDX_BITS + C.TAG_BITS == 64 and C.LOOKUP_MAX + 1 < 1 << C.IDX_BITS  # index + 1 fits its field
    assert '#include "mox_wordset.h"' in src and '#include "mox_wordhash.h"' in ws
    assert "fnv_finish" in _read("map-oxidize_amd", "csrc", "mox_wordhash.h")  # the forced-collision build truncates the hash
    for k in ("k_lk_build", "k_lk_stream"):
        assert re.search(r'^extern "C" __global__ __launch_bounds__\(WS_T\) void %s\(.*\) \{ ws_\w+<LkWords>\(.*\); \}$' % k, src, re.M), k
    op_objects("lookup", hc=True)  # mox_lookup_hc.o (KERNEL_FLAGS and HC_FLAGS) in libmox_hc.so, mox_lookup.o in the two others


def test_sum_lookups():
    a, b, c = [3, 0, 0, 5], [0, 0, 7, 0], [0, 0, 0, 0]
    got = mdist.sum_lookups([a, b, c])
    assert got.dtype == np.uint64 and got.tolist() == [3, 0, 7, 5]
    assert mdist.sum_lookups([np.array(a, np.uint64)]).tolist() == a
    assert mdist.sum_lookups([]).size == 0 and mdist.sum_lookups([[], []]).size == 0
    big = (1 << 64) - 1
    assert mdist.sum_lookups([[big, 1 << 63], [0, 1 << 62]]).tolist() == [big, (1 << 63) + (1 << 62)]
    with pytest.raises(ValueError):
        mdist.sum_lookups([a, b[:3]])


def test_sum_lookups_ownership():
    a, b = [3, 0, 0, 0], [0, 0, 7, 0]
    fa, fb = [True, False, False, True], [False, False, True, False]  # (a count-0 word is found, too)
    assert mdist.sum_lookups([a, b], found=[fa, fb]).tolist() == [3, 0, 7, 0]
    with pytest.raises(ValueError):
        mdist.sum_lookups([a, b], found=[fa, [True, False, True, False]])  # word 0 on both ranks
    with pytest.raises(ValueError):
        mdist.sum_lookups([a, b], found=[fa])  # a mask per rank
    with pytest.raises(ValueError):
        mdist.sum_lookups([a, b], found=[fa, fb[:3]])


def test_expected_on_a_hand_written_example():
    items = [(b"b", 5), (b"a", 2), (b"zero", 0), (b"ab\x00", 9)]
    queries = [b"a", b"zz", b"zero", b"a", b"ab", b"ab\x00", b"", b"B"]
    counts, index = C.expected(items, queries)
    assert counts == [2, 0, 0, 2, 0, 9, 0, 0]
    assert index == [1, C.NONE, 2, 1, C.NONE, 3, C.NONE, C.NONE]
    assert C.expected([], [b"a"]) == ([0], [C.NONE]) and C.expected(items, []) == ([], [])


def test_case_tables_have_their_shapes():
    assert set(C.TABLE_NS) >= {1, 2, 63, 64, 65, 255, 256, 257, C.TILE - 1, C.TILE, C.TILE + 1}
    tiles = (C.STRIDE_N + C.TILE - 1) // C.TILE
    assert tiles >= 3 * C.STRIDE_GRID and C.STRIDE_N % C.TILE == 1  # three strides per workgroup, a one-word last tile
    assert C.QUERY_NS == (0, 1, 2, 63, 64, 65, 1023, 1024, 1025)
    w, c = C.table_words(5000, 3)
    assert len(set(w)) == 5000 and sorted(c) == list(range(1, 5001))
    assert {len(x) for x in w} >= set(range(3, 25)) and any(len(x) > 16 for x in w)
    q = C.present_and_absent(w, 4)
    assert len(q) == 10000 and len(set(q)) == 10000 and set(w) < set(q)
    assert not set(C.absent_words(5000)) & set(w)


def test_shape_table_shapes():
    w, c = C.shape_table()
    assert len(set(w)) == len(w) == len(c)
    lens = {len(x) for x in w}
    assert lens >= set(range(1, 41)) | set(C.SHAPE_LENS) | set(range(1, 71)) and max(lens) == 100000
    assert {7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65} == set(C.SHAPE_LENS)
    assert all(x in w for x in C.NUL_WORDS + C.PREFIX_CHAIN) and all(b"\x00" in x for x in C.NUL_WORDS)
    assert sum(any(b > 127 for b in x) for x in w) >= 5
    assert C.near_misses(b"ab") == [b"a", b"aba", b"ab\x00", b"ac", b"AB"]
    assert C.near_misses(b"7") == [b"", b"7a", b"7\x00", b"6"]  # (upper() of a digit is the digit)
    q = C.shape_queries(w)
    assert set(w) < set(q) and b"" in q and len(q) > 5 * len(w)
    tw = set(w)
    # w + "a", w + NUL and w.upper() are absent for nearly every word; "r176" and "r1763" next to "r1762" are table words
    assert sum(x not in tw for x in q) > 2 * len(w)
    assert sum(x in tw for x in q) > len(w) + 1000
    assert any(x in tw for x in C.near_misses(b"a" * 10))  # the chain's near misses are table words, too
    w1, c1 = C.last_is_one_byte()
    assert max(w1) == b"~" and len(set(w1)) == len(w1) == len(c1)


def test_collide_table_shapes():
    w, c, q = C.collide_table()
    assert len(set(w)) == 4000 == len(c) and len(q) == 2000 == len(set(q))
    tw = set(w)
    assert sum(x in tw for x in q) == 1000
    assert sum(len(x) > C.LANE_MAX for x in w) == 400
    assert sum(len(x) > C.LANE_MAX for x in q if x in tw) > 50 and sum(len(x) > C.LANE_MAX for x in q if x not in tw) == 100


def test_fixed_width_queries():
    mat, offs = C.fixed_width_queries(1 << 12)
    assert mat.shape == (1 << 12, 6) and offs.tolist() == list(range(0, 6 * (1 << 12) + 1, 6))
    words = [mat[i].tobytes() for i in range(1 << 12)]
    assert len(set(words)) == 1 << 12 and all(C.fixed_width_number(w) == i for i, w in enumerate(words))
    mat, _ = C.fixed_width_queries(C.LOOKUP_MAX)
    assert np.unique(mat.view("S6").ravel()).size == C.LOOKUP_MAX
    assert C.fixed_width_number(mat[C.LOOKUP_MAX - 1].tobytes()) == C.LOOKUP_MAX - 1


def test_cli_documents_the_flag():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--word"' in src and "mox_lookup_words" in src and 'printf("Counts:\\n")' in src


def test_docs_mention_the_lookup():
    for doc, words in (("README.md", ["mox_lookup_words", "--word"]),
                       ("DESIGN.md", ["mox_lookup.hip", "k_lk_stream", "Device lookup against the fetch it replaces"]),
                       ("INTEGRATION.md", ["mox_lookup_words", "mox_lookup_info"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
