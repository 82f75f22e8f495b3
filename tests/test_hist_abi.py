"""CPU: the surface of the device histograms (include/mox.h mox_hist_result /
mox_hist_free, the Python mirror, the dist helper, the command-line option)
and the model and case tables of test_gpu_hist.py (hist_cases.py).  No GPU
code runs here."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hist_cases as C
import mox
import rank_cases
from conftest import ROOT
from srcpins import _read, code_only, op_objects
from mox import dist


KERNELS = ("k_hg_keys", "k_hg_count", "k_hg_scan", "k_hg_bins", "k_hg_diff")
RANK_KERNELS = ("k_rk_max", "k_rk_hist", "k_rk_scan_part", "k_rk_scan_top", "k_rk_scan_apply", "k_rk_scatter", "k_rk_len", "k_rk_offs",
                "k_rk_emit")


def test_header_declares_the_histogram():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_HIST_COUNT 0u", "#define MOX_HIST_BYTES 1u", "#define MOX_HIST_CHARS 2u", "#define MOX_HIST_FIRST 3u",
              "#define MOX_HIST_RANGE 0x1u", "#define MOX_HIST_MAX_WORDS 0xFFFFFFFFull"):
        assert d in src, d
    assert "int mox_hist_result(mox_engine* e, const mox_hist* h, mox_hist_table** out, mox_hist_info* info );" in src
    assert "void mox_hist_free(mox_hist_table* t);" in src
    m = re.search(r"typedef struct mox_hist \{(.*?)\} mox_hist;", src)
    assert [d.strip() for d in m.group(1).split(";") if d.strip()] == ["uint32_t key, flags", "uint64_t first, rows", "uint64_t reserved[4]"]
    m = re.search(r"typedef struct mox_hist_table \{(.*?)\} mox_hist_table;", src)
    assert [d.strip() for d in m.group(1).split(";") if d.strip()] == [
        "uint64_t n", "uint64_t words, tokens", "const uint64_t* keys", "const uint64_t* bin_words", "const uint64_t* bin_tokens",
        "const uint64_t* first_row"]
    m = re.search(r"typedef struct mox_hist_info \{(.*?)\} mox_hist_info;", src)
    assert [d.strip() for d in m.group(1).split(";") if d.strip()] == [
        "uint64_t words, tokens, bins, max_key, digit_passes, device_bytes", "double ms", "uint64_t reserved[4]"]
    # the section follows the search's and the contract is written down next to the declarations
    head = "histograms of the device-resident result"
    assert raw.index("searching the sorted device-resident result") < raw.index(head) < raw.index("int mox_get_stats")
    doc = re.sub(r"\s*\n \*\s+", " ", raw.split(head)[1].split("int mox_get_stats")[0])  # (the comment's line breaks)
    for phrase in ("only reads", "MOX_F_SORT_BYTES or not", "accumulator", "member 0", "4 x bins", "nothing runs on the device",
                   "no radix pass", "keys[i] * bin_words[i] mod 2^64", "inconsistent totals", "contiguous row ranges", "mox_fetch_rows",
                   "mox_exchange", "first_row is per rank", "never read a word byte", "at most 4 bytes", "big-endian", "bits 39..8",
                   "a proper prefix first", "An empty word's key is 0", "MOX_ESTATE", "MOX_EINVAL", "MOX_ENOMEM", "untouched",
                   "MOX_HIST_GRID", "MOX_TEST_FAIL_HIST", "mox_hist_free", "no cap on bins"):
        assert phrase in doc, phrase


def test_python_mirror_has_the_c_layout(tmp_path):
    """sizeof and every field offset of mox_hist, mox_hist_info and mox_hist_table, from a probe compiled against the header."""
    structs = (("mox_hist", mox.Hist, 56), ("mox_hist_info", mox.HistInfo, 88), ("mox_hist_table", mox._HistTable, 56))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {"]
    for name, cls, _ in structs:
        lines.append('  printf("%s.size %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines += ['  printf("keys %u %u %u %u\\n", MOX_HIST_COUNT, MOX_HIST_BYTES, MOX_HIST_CHARS, MOX_HIST_FIRST);',
              '  printf("range %u\\n", MOX_HIST_RANGE);', '  printf("max %llu\\n", (unsigned long long)MOX_HIST_MAX_WORDS);',
              "  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split(None, 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, cls, size in structs:
        assert int(got[name + ".size"]) == ctypes.sizeof(cls) == size, name
        for field, _ in cls._fields_:
            assert int(got["%s.%s" % (name, field)]) == getattr(cls, field).offset, (name, field)
    assert [int(x) for x in got["keys"].split()] == [mox.HIST_COUNT, mox.HIST_BYTES, mox.HIST_CHARS, mox.HIST_FIRST] == \
        [C.COUNT, C.BYTES, C.CHARS, C.FIRST]
    assert int(got["range"]) == mox.HIST_RANGE == C.RANGE
    assert int(got["max"]) == mox.HIST_MAX_WORDS == C.MAX_WORDS == (1 << 32) - 1


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_both_symbols(path):
    raw = ctypes.CDLL(path)
    assert hasattr(raw, "mox_hist_result") and hasattr(raw, "mox_hist_free")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_hist_result
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.POINTER(mox.Hist), ctypes.POINTER(ctypes.POINTER(mox._HistTable)),
                                ctypes.POINTER(mox.HistInfo)]
    g = L.mox_hist_free
    assert g.restype is None and list(g.argtypes) == [ctypes.POINTER(mox._HistTable)]


def test_argument_checks_touch_no_device_and_leave_the_outputs():
    L = mox.lib()
    info = mox.HistInfo(words=5, tokens=6, bins=7, max_key=8, digit_passes=9, device_bytes=10)
    out = ctypes.POINTER(mox._HistTable)()

    def call(engine, h, o=out):
        return L.mox_hist_result(engine, ctypes.byref(h) if h is not None else None, ctypes.byref(o) if o is not None else None,
                                 ctypes.byref(info))

    assert call(None, mox.Hist()) == mox.MOX_EINVAL and b"NULL" in L.mox_last_error()
    # every argument check comes before the engine is looked at (no device is touched: this handle is no engine)
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert call(bogus, None) == mox.MOX_EINVAL and call(bogus, mox.Hist(), None) == mox.MOX_EINVAL
    assert call(bogus, mox.Hist(key=4)) == mox.MOX_EINVAL and b"key" in L.mox_last_error()
    assert call(bogus, mox.Hist(flags=2)) == mox.MOX_EINVAL and b"flags" in L.mox_last_error()
    assert call(bogus, mox.Hist(flags=0x80000001)) == mox.MOX_EINVAL
    for i in range(4):
        h = mox.Hist()
        h.reserved[i] = 1
        assert call(bogus, h) == mox.MOX_EINVAL and b"reserved" in L.mox_last_error()
    assert call(bogus, mox.Hist(first=1)) == mox.MOX_EINVAL and b"MOX_HIST_RANGE" in L.mox_last_error()
    assert call(bogus, mox.Hist(rows=1)) == mox.MOX_EINVAL
    assert not out
    assert (info.words, info.tokens, info.bins, info.max_key, info.digit_passes, info.device_bytes) == (5, 6, 7, 8, 9, 10)
    L.mox_hist_free(None)  # NULL is fine


def test_python_surface():
    p = inspect.signature(mox.Engine.histogram).parameters
    assert list(p)[1:] == ["key", "first", "n", "with_info"]
    assert [p[k].default for k in list(p)[1:]] == ["count", None, None, False]
    assert [f for f, _ in mox.HistInfo._fields_] == ["words", "tokens", "bins", "max_key", "digit_passes", "device_bytes", "ms", "reserved"]
    assert mox._HIST_KEYS == dict(zip(C.KEYS, (C.COUNT, C.BYTES, C.CHARS, C.FIRST)))
    for w in C.FIRST_WORDS + [b""]:
        assert mox.hist_first_bytes(C.key_first(w, 0)) == C.first_window(w)
    assert mox.hist_first_bytes(np.uint64((0xE282AC << 16) | 3)) == "€".encode()


def test_constants_and_kernels_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_hist.hip")
    t = int(re.search(r"^constexpr int HG_T = (\d+);", src, re.M).group(1))
    rounds = int(re.search(r"^constexpr int HG_ROUNDS = (\d+);", src, re.M).group(1))
    assert re.search(r"^constexpr uint32_t HG_TILE = HG_T \* HG_ROUNDS;", src, re.M)
    assert t == C.ROUND and t * rounds == C.TILE == rank_cases.TILE and t % 64 == 0  # the sort's tiles are the same rows
    assert 'static_assert(HG_TILE == %d, "tests/hist_cases.py TILE");' % C.TILE in src
    assert int(re.search(r"^constexpr int HG_TOP_T = (\d+);", src, re.M).group(1)) == C.TOP_STEP
    assert int(re.search(r"^constexpr uint32_t HG_LANE_MAX = (\d+);", src, re.M).group(1)) == C.LANE_MAX
    for k in KERNELS:
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
    assert set(re.findall(r"\b(k_hg_\w+)\(", src)) == set(KERNELS)
    # the LDS list of long words only: no global atomic places a bin or adds a count; and no workgroup waits on another
    device = src.split('extern "C" void mox_hist_free(')[0]  # (the kernels: the entry points start there)
    assert set(re.findall(r"atomic\w+\(&?([\w.>-]+)", src)) == {"s_nbig"} and "__shared__ uint32_t s_nbig;" in device
    assert not re.search(r"\bwhile\b|s_sleep|__threadfence|volatile", device)
    assert 'grid_cap(e, "MOX_HIST_GRID")' in src and 'test_fail_hook("MOX_TEST_FAIL_HIST")' in src
    # one sort: the ranking's, through rank_order
    assert "rank_order(e, keys_in, n, 0, cap, 0, &ro)" in src and "k_rk_" not in re.sub(r"//.*", "", src)
    report = src.split("#include")[0].split("Resource usage")[1]
    for k in KERNELS:
        assert re.search(r"%s\s+\d+ VGPRs, \d+ SGPRs,\s+\d+ B LDS, no scratch, no spills" % k, report), k


def test_the_ranking_shares_its_sort_and_keeps_its_kernels():
    src = _read("map-oxidize_amd", "csrc", "mox_rank.hip")
    assert set(re.findall(r"\b(k_rk_\w+)\(", src)) == set(RANK_KERNELS)
    for k in RANK_KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(%s," % k, src)) == 1, k  # every kernel is launched from one place
    assert len(re.findall(r"^int rank_order\(", src, re.M)) == 1 and src.count("rank_order(e, T.counts, T.n, flip, cap, ") == 1
    host = _read("map-oxidize_amd", "csrc", "mox_host.h")
    assert ("int rank_order(mox_engine* e, const uint64_t* d_keys, uint64_t n, uint64_t flip, uint64_t cap, size_t extra, "
            "RankOrder* out);") in host
    assert "struct RankOrder {" in host and "DevBuf hg_tmp, hg_out, hg_pin;" in host  # (freed: test_result_buffers.py)
    for name in ("mox_dev.h", "mox_host.h"):
        assert "mox_hist.hip" in _read("map-oxidize_amd", "csrc", name).split("#pragma once")[0], name


def test_makefile_puts_one_object_into_all_three_libraries():
    op_objects("hist", hc=False)  # no mox_hist_hc.o, no mox_hist_check.o; KERNEL_FLAGS; once per library


def test_keys_on_hand_written_words():
    def first(w):
        return C.key_first(w, 0)

    assert first(b"a") == (0x61 << 32) | 1
    assert first("é".encode()) == (0xC3 << 32) | (0xA9 << 24) | 2
    assert first("€".encode()) == (0xE2 << 32) | (0x82 << 24) | (0xAC << 16) | 3
    assert first("😀".encode()) == (0xF0 << 32) | (0x9F << 24) | (0x98 << 16) | (0x80 << 8) | 4
    assert first(b"\x80\x80a") == (0x80 << 32) | (0x80 << 24) | 2  # a 2-byte window: the continuation bytes stay
    assert first(b"\x80" * 5) == (0x80808080 << 8) | 4             # capped at 4
    assert first(b"ab") == first(b"a") and first("€uro".encode()) == first("€".encode()) and first(b"") == 0
    assert first(b"\x00") == 1 and first(b"\x00\x80") == (0x80 << 24) | 2
    # ascending keys: the windows in bytewise order, a proper prefix first
    wins = [C.first_window(w) for w in C.FIRST_WORDS]
    assert sorted(set(wins), key=lambda w: C.key_first(w, 0)) == sorted(set(wins))
    assert [C.key_chars(w, 0) for w in (b"a", "é".encode(), "€".encode(), "😀".encode(), b"\x80\x80a", b"\x80" * 5)] == [1, 1, 1, 1, 1, 0]
    assert C.key_chars("naïve €5".encode(), 0) == 8 and C.key_bytes("naïve €5".encode(), 0) == 11
    assert C.key_chars(C.TWO_BYTE_BIG, 0) == 50000 and len(C.TWO_BYTE_BIG) == 100000
    assert C.key_count(b"x", 7) == 7


def test_expected_on_hand_written_cases():
    items = [(b"the", 9), (b"un", 2), ("été".encode(), 0), (b"u", 9), (b"max", C.U64), (b"b", 2), ("€".encode(), 1), (b"a", 2)]
    assert C.expected(items, "count") == [(0, 1, 0, 2), (1, 1, 1, 6), (2, 3, 6, 1), (9, 2, 18, 0), (C.U64, 1, C.U64, 4)]
    assert C.expected(items, "bytes") == [(1, 3, 13, 3), (2, 1, 2, 1), (3, 3, (10 + C.U64) & C.U64, 0), (5, 1, 0, 2)]
    assert C.expected(items, "chars") == [(1, 4, 14, 3), (2, 1, 2, 1), (3, 3, (9 + C.U64) & C.U64, 0)]
    e = C.expected(items, "first")
    assert [mox.hist_first_bytes(k) for k, _, _, _ in e] == [b"a", b"b", b"m", b"t", b"u", "é".encode(), "€".encode()]
    assert e[4] == (C.key_first(b"u", 0), 2, 11, 1)
    # ranges: first_row stays absolute; the end is clipped; first past the end is the empty range
    assert C.expected(items, "count", 3, 3) == [(2, 1, 2, 5), (9, 1, 9, 3), (C.U64, 1, C.U64, 4)]
    assert C.expected(items, "count", 5, C.U64) == [(1, 1, 1, 6), (2, 2, 4, 5)]
    assert C.expected(items[5:], "count") == [(1, 1, 1, 1), (2, 2, 4, 0)]
    assert C.expected(items, "count", 8, 5) == [] == C.expected(items, "bytes", 0, 0) == C.expected([], "first")
    assert C.expected([(b"x", C.U64)] * 3, "count") == [(C.U64, 3, (3 * C.U64) & C.U64, 0)]  # the wrap
    assert C.info_of(C.expected(items, "count")) == {"words": 8, "tokens": (25 + C.U64) & C.U64, "bins": 5, "max_key": C.U64,
                                                     "digit_passes": 8}
    assert C.info_of([]) == {"words": 0, "tokens": 0, "bins": 0, "max_key": 0, "digit_passes": 0}
    assert C.info_of(C.expected([(b"x", 0)], "count"))["digit_passes"] == 0


def test_case_tables_have_their_shapes():
    assert C.TABLE_NS == (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
    tiles = (C.STRIDE_N + C.TILE - 1) // C.TILE
    assert tiles == 3 * C.STRIDE_GRID + 1 and C.STRIDE_N % C.TILE == 1
    words, counts = C.utf8_words()
    assert len(set(words)) == len(words) == len(counts) and set(C.FIRST_WORDS) <= set(words)
    assert {len(C.first_window(w)) for w in words} == {1, 2, 3, 4}
    assert any(is_c for is_c in (C.is_cont(w[0]) for w in words)) and any(0 in w for w in words)
    lens = {len(w) for w in words}
    assert {1, 63, 64, 65, 66, 100000} <= lens and C.TWO_BYTE_BIG in words
    # a multi-byte character lies across an 8-byte step of the count, and across the lane / wave edge
    assert any(not C.is_cont(w[7]) and C.is_cont(w[8]) for w in words if len(w) > 8)
    assert any(len(w) > C.LANE_MAX and C.is_cont(w[64]) for w in words)
    assert len({C.key_chars(w, 0) for w in words}) > 20 and 0 in {C.key_chars(w, 0) for w in words}


def test_sum_histograms_merges_by_key():
    def part(keys, words, tokens):
        return tuple(np.array(a, dtype=np.uint64) for a in (keys, words, tokens)) + (np.zeros(len(keys), np.uint64), 0, 0)

    a = part([1, 2, 9], [5, 1, 2], [5, 2, C.U64])
    b = part([0, 2, 9, 70000], [1, 4, 1, 1], [0, 8, 3, 70000])
    keys, words, tokens, n_words, n_tokens = dist.sum_histograms([a, b])
    assert keys.dtype == np.uint64 and keys.tolist() == [0, 1, 2, 9, 70000]
    assert words.tolist() == [1, 5, 5, 3, 1] and tokens.tolist() == [0, 5, 10, 2, 70000]  # (the sum wraps as the device's)
    assert n_words == 15 and n_tokens == (5 + 2 + C.U64 + 8 + 3 + 70000) & C.U64
    keys, words, tokens, n_words, n_tokens = dist.sum_histograms([a])
    assert keys.tolist() == [1, 2, 9] and words.tolist() == [5, 1, 2] and n_tokens == (7 + C.U64) & C.U64
    keys, words, tokens, n_words, n_tokens = dist.sum_histograms([])
    assert keys.size == words.size == tokens.size == 0 and (n_words, n_tokens) == (0, 0)
    with pytest.raises(ValueError):
        dist.sum_histograms([a, (a[0], a[1][:2], a[2])])


def test_cli_documents_the_option():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--histogram"' in src and "mox_hist_result" in src and "mox_hist_free" in src
    assert "--histogram KEY" in src.split("#include")[0]


def test_docs_mention_the_histograms():
    for doc, words in (("README.md", ["mox_hist_result", "Engine.histogram", "--histogram"]),
                       ("DESIGN.md", ["Histograms of the result", "mox_hist.hip", "k_hg_bins", "rank_order", "run-length",
                                      "no cap on bins", "two-dimensional", "Good–Turing",
                                      "Device histogram against fetch + host histogram"]),
                       ("INTEGRATION.md", ["mox_hist_result", "mox_hist_info", "mox_hist_table", "mox_hist_free"]),
                       (os.path.join("tools", "README.md"), ["hist_timing.py"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
