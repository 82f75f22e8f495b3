"""CPU: the surface of the device search of the sorted result (include/mox.h
mox_find_ranges / mox_top_rows, the Python mirror, the dist helper, the
command-line option) and the model and case tables of test_gpu_find.py
(find_cases.py).  No GPU code runs here."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

import find_cases as C
import mox
from conftest import ROOT
from srcpins import _read, code_only, op_objects
from mox import dist


KERNELS = ("k_fd_search", "k_fd_tiles", "k_fd_scan", "k_fd_sum")


def test_header_declares_the_search_and_the_row_top_k():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_FIND_EXACT 0u", "#define MOX_FIND_PREFIX 1u", "#define MOX_FIND_LOWER 2u", "#define MOX_FIND_MAX (1u << 20)"):
        assert d in src, d
    assert ("int mox_find_ranges(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint32_t mode, "
            "uint64_t* first, uint64_t* last, uint64_t* sums , mox_find_info* info );") in src
    assert "int mox_top_rows(mox_engine* e, uint64_t first, uint64_t n, size_t k, mox_table** out);" in src
    m = re.search(r"typedef struct mox_find_info \{(.*?)\} mox_find_info;", src)
    assert [d.strip() for d in m.group(1).split(";") if d.strip()] == [
        "uint64_t queries, matched", "uint64_t rows", "uint64_t tile_pass", "uint64_t device_bytes", "double ms", "uint64_t reserved[4]"]
    # the contract is written down next to the declaration
    doc = raw.split("searching the sorted device-resident result")[1].split("int mox_get_stats")[0]
    for phrase in ("MOX_ESTATE", "mox_sort_result", "untouched", "MOX_FIND_GRID", "mox_fetch_rows", "MOX_EINVAL", "MOX_ENOMEM",
                   "insertion point", "wrapping", "sums == NULL no kernel reads a count", "member 0", "Rust String Ord"):
        assert phrase in doc, phrase


def test_python_mirror_has_the_c_layout(tmp_path):
    """sizeof and every field offset of mox_find_info, from a probe compiled against the header."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mox_find_info));']
    for field, _ in mox.FindInfo._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(mox_find_info, %s));' % (field, field))
    lines += ['  printf("modes %u %u %u\\n", MOX_FIND_EXACT, MOX_FIND_PREFIX, MOX_FIND_LOWER);', '  printf("max %u\\n", MOX_FIND_MAX);',
              "  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split(None, 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(mox.FindInfo) == 80
    for field, _ in mox.FindInfo._fields_:
        assert int(got[field]) == getattr(mox.FindInfo, field).offset, field
    assert [int(x) for x in got["modes"].split()] == [mox.FIND_EXACT, mox.FIND_PREFIX, mox.FIND_LOWER] == [C.EXACT, C.PREFIX, C.LOWER]
    assert int(got["max"]) == mox.FIND_MAX == C.FIND_MAX == 1 << 20


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_both_symbols(path):
    raw = ctypes.CDLL(path)
    assert hasattr(raw, "mox_find_ranges") and hasattr(raw, "mox_top_rows")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    U64, U64P, VP = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    f = L.mox_find_ranges
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [VP, VP, U64P, U64, ctypes.c_uint32, U64P, U64P, U64P, ctypes.POINTER(mox.FindInfo)]
    g = L.mox_top_rows
    assert g.restype is ctypes.c_int and list(g.argtypes) == [VP, U64, U64, ctypes.c_size_t, ctypes.POINTER(ctypes.POINTER(mox._Table))]


def test_null_engine_is_einval_and_leaves_the_outputs():
    L = mox.lib()
    U64P = ctypes.POINTER(ctypes.c_uint64)
    offs = np.array([0, 1, 2], dtype=np.uint64)
    first, last, sums = (np.full(2, v, dtype=np.uint64) for v in (11, 12, 13))
    info = mox.FindInfo(queries=5, matched=6, rows=7, tile_pass=8, device_bytes=9)
    rc = L.mox_find_ranges(None, ctypes.c_char_p(b"ab"), offs.ctypes.data_as(U64P), 2, mox.FIND_PREFIX, first.ctypes.data_as(U64P),
                           last.ctypes.data_as(U64P), sums.ctypes.data_as(U64P), ctypes.byref(info))
    assert rc == mox.MOX_EINVAL and b"NULL" in L.mox_last_error()
    assert first.tolist() == [11, 11] and last.tolist() == [12, 12] and sums.tolist() == [13, 13]
    assert (info.queries, info.matched, info.rows, info.tile_pass, info.device_bytes) == (5, 6, 7, 8, 9)
    t = ctypes.POINTER(mox._Table)()
    assert L.mox_top_rows(None, 0, 1, 1, ctypes.byref(t)) == mox.MOX_EINVAL and not t


def test_python_surface():
    p = inspect.signature(mox.Engine.find).parameters
    assert list(p)[1:] == ["keys", "mode", "with_sums", "with_info"]
    assert [p[k].default for k in list(p)[2:]] == ["prefix", True, False]
    p = inspect.signature(mox.Engine.find_packed).parameters
    assert list(p)[1:] == ["data", "offs", "mode", "with_sums", "with_info"]
    p = inspect.signature(mox.Engine.top_rows).parameters
    assert list(p)[1:] == ["first", "n", "k"] and p["k"].default == 10
    p = inspect.signature(mox.Engine.complete).parameters
    assert list(p)[1:] == ["prefix", "k"] and p["k"].default == 10
    assert [f for f, _ in mox.FindInfo._fields_] == ["queries", "matched", "rows", "tile_pass", "device_bytes", "ms", "reserved"]


def test_model_agrees_with_a_brute_force_scan():
    """expected() -- bisect and the prefix's successor -- against the definition, on random byte strings over a
    small alphabet that holds 0x00 and 0xFF (many shared prefixes, many keys that are table words)."""
    rng = random.Random(17)
    alphabet = (0x00, 0x01, 0x61, 0x7F, 0x80, 0xFF)

    def word():
        return bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 5)))

    for _ in range(20):
        items = sorted({word(): rng.randint(0, C.U64) for _ in range(rng.randint(0, 120))}.items())
        keys = [word() for _ in range(80)] + [b"", b"\xff", b"\xff\xff", b"\x00"] + [w for w, _ in items[:20]]
        for _, mode in C.MODES:
            assert C.expected(items, keys, mode) == C.brute(items, keys, mode)
    assert C.prefix_end(b"") is None and C.prefix_end(b"\xff\xff") is None
    assert C.prefix_end(b"a\xff") == b"b" and C.prefix_end(b"ab") == b"ac"


def test_model_on_hand_written_cases():
    items = [(b"ab", 3), (b"ab\x00", 4), (b"abc", C.U64), (b"b", 1), (b"\xff", 2)]
    assert C.expected(items, [b"ab", b"a", b"", b"abd", b"\xff", b"c"], C.PREFIX) == (
        [0, 0, 0, 3, 4, 4], [3, 3, 5, 3, 5, 4], [6, 6, 9, 0, 2, 0])
    assert C.expected(items, [b"ab", b"ab\x00", b"a", b"zz"], C.EXACT) == ([0, 1, 0, 4], [1, 2, 0, 4], [3, 4, 0, 0])
    assert C.expected(items, [b"ab", b"ac", b"\xff\x00"], C.LOWER) == ([0, 3, 5], [0, 3, 5], [0, 0, 0])
    assert C.info_of([0, 3, 4], [3, 3, 5]) == {"queries": 3, "matched": 2, "rows": 4}
    assert C.top_of([(b"a", 2), (b"b", 9), (b"c", 9), (b"d", 1)], 1, 4, 2) == [(b"b", 9), (b"c", 9)]
    assert [C.holds_tile(a, b) for a, b in ((1024, 2048), (1023, 2049), (1, 1023), (1000, 1030), (0, 1024), (1, 2047), (0, 0))] == \
        [True, True, False, False, True, False, False]


def test_case_tables_have_their_shapes():
    assert C.TABLE_NS == (0, 1, 2, 1023, 1024, 1025, 2049, 5121)
    tiles = (C.STRIDE_N + C.TILE - 1) // C.TILE
    assert tiles == 3 * C.STRIDE_GRID and C.STRIDE_N == 5121
    words, counts = C.table_words(300, 1)
    assert len(set(words)) == 300 == len(counts) and any(w[0] > 0x7F for w in words) and any(len(w) > 16 for w in words)
    assert set(C.EDGE_LENS) == set(range(19)) | {63, 64, 65, 300}
    words, counts = C.edge_table()
    assert {len(w) for w in words} >= set(C.EDGE_LENS) - {0} and b"ab" in words and b"ab\x00" in words
    for p in C.EDGE_POS:
        assert {w[p] for w in words if len(w) == 12} >= set(C.EDGE_BYTES)
    assert len([w for w in words if len(w) == 200 and w[:199] == b"z" * 199]) == 7
    keys = C.edge_keys(words)
    assert b"" in keys and {len(k) for k in keys} >= set(C.EDGE_LENS) and set(words) <= set(keys)
    # the groups give the ranges they are named for
    for groups, ranges in ((C.TILE_GROUPS_A, C.TILE_RANGES_A), (C.TILE_GROUPS_B, C.TILE_RANGES_B)):
        words, counts = C.group_table(groups, 2)
        items = sorted(zip(words, counts))
        first, last, _ = C.expected(items, [k for k, _, _ in ranges], C.PREFIX)
        assert list(zip(first, last)) == [(a, b) for _, a, b in ranges]
    assert [C.holds_tile(a, b) for _, a, b in C.TILE_RANGES_A] == [False, True, True, True, False]
    assert sum(C.WRAP_COUNTS) > 2 * C.U64 and {0, 1, C.U64} <= set(C.WRAP_COUNTS)


def test_sum_finds_adds_its_inputs():
    a = (np.array([0, 5, 7], np.uint64), np.array([3, 5, 9], np.uint64), np.array([10, 0, C.U64], np.uint64))
    b = (np.array([2, 2, 0], np.uint64), np.array([2, 4, 1], np.uint64), np.array([0, 7, 2], np.uint64))
    rows, sums = dist.sum_finds([a, b])
    assert rows.dtype == np.uint64 and rows.tolist() == [3, 2, 3] and sums.tolist() == [10, 7, 1]  # (the sum wraps as the device's)
    rows, sums = dist.sum_finds([a[:2], b])
    assert rows.tolist() == [3, 2, 3] and sums is None
    rows, sums = dist.sum_finds([])
    assert rows.size == 0 and sums.size == 0
    with pytest.raises(ValueError):
        dist.sum_finds([a, tuple(x[:2] for x in b)])


def test_constants_and_kernels_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_find.hip")
    assert int(re.search(r"^constexpr uint64_t FD_TILE = (\d+);", src, re.M).group(1)) == C.TILE
    assert int(re.search(r"^constexpr int FD_T = (\d+);", src, re.M).group(1)) == 256
    for k in KERNELS:
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
    assert set(re.findall(r"\b(k_fd_\w+)\(", src)) == set(KERNELS)
    # no atomic touches a count or an output: the error word only; and no workgroup waits on another
    assert set(re.findall(r"atomic\w+\(&?([\w.>-]+)", src)) == {"K.ctl->err"}
    assert not re.search(r"\bwhile\b|s_sleep|__threadfence|volatile", src.split('extern "C" int mox_find_ranges(')[0])  # (the kernels: the host side starts there)
    assert 'grid_cap(e, "MOX_FIND_GRID")' in src and "sort_for_fetch(e, &host_sort)" in src
    report = src.split("#include")[0].split("Resource usage")[1]
    for k in KERNELS:
        assert re.search(r"%s\s+\d+ VGPRs, \d+ SGPRs,\s+\d+ B LDS, no scratch, no spills" % k, report), k
    op_objects("find", hc=False)  # no mox_find_hc.o, no mox_find_check.o; KERNEL_FLAGS; once per library
    host = _read("map-oxidize_amd", "csrc", "mox_host.h")
    assert "DevBuf fd_tmp, fd_pin;" in host  # (freed: test_result_buffers.py)
    assert "int sort_for_fetch(mox_engine* e, bool* host_sort);" in host  # exposed, not copied
    engine = _read("map-oxidize_amd", "csrc", "mox_engine.hip")
    assert len(re.findall(r"^int sort_for_fetch\(", engine, re.M)) == 1
    # mox_top_words and mox_top_rows share one body
    topk = _read("map-oxidize_amd", "csrc", "mox_topk.hip")
    assert topk.count("top_of_rows(e, ") == 2 and topk.count("k_tk_sort, dim3(1)") == 1


def test_cli_documents_the_option():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--prefix"' in src and "mox_find_ranges" in src and "mox_top_rows" in src
    assert "--prefix" in src.split("#include")[0]


def test_docs_mention_the_search():
    for doc, words in (("README.md", ["mox_find_ranges", "mox_top_rows", "--prefix"]),
                       ("DESIGN.md", ["Searching the sorted result", "mox_find.hip", "k_fd_search",
                                      "Device search against the streamed lookup"]),
                       (os.path.join("tools", "README.md"), ["find_timing.py"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
