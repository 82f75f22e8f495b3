"""CPU: the surface of the device ranking and the row fetch (include/mox.h
mox_rank_result / mox_fetch_rows, the Python mirror, the command-line option)
and the case tables of test_gpu_rank.py (rank_cases.py).  No GPU code runs
here."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import mox
import rank_cases as C
from conftest import ROOT
from srcpins import _read, code_only, op_objects, struct_fields


KERNELS = ("k_rk_max", "k_rk_hist", "k_rk_scan_part", "k_rk_scan_top", "k_rk_scan_apply", "k_rk_scatter", "k_rk_len", "k_rk_offs",
           "k_rk_emit")


def test_header_declares_the_ranking_and_the_row_fetch():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_RANK_ASCENDING 0x1u", "#define MOX_RANK_MAX_WORDS 0xFFFFFFFFull"):
        assert d in src, d
    assert "int mox_rank_result(mox_engine* e, uint32_t flags, mox_rank_info* info );" in src
    assert "int mox_fetch_rows(mox_engine* e, uint64_t first, uint64_t n, mox_table** out);" in src
    assert struct_fields(src, "mox_rank_info") == [
        ("uint64_t", "words"), ("uint64_t", "tokens"), ("uint64_t", "max_count"), ("uint64_t", "digit_passes"),
        ("uint64_t", "device_bytes"), ("double", "ms"), ("uint64_t", "reserved[4]")]
    # the section follows the filter's and the contract is written down next to the declarations
    head = "ranking the device-resident result by count"
    assert raw.index("filtering the device-resident result") < raw.index(head) < raw.index("int mox_get_stats")
    doc = raw.split(head)[1].split("mox_get_stats")[0]
    for phrase in ("stable", "mox_top_words(k)", "count descending, then bytewise", "full u64", "MOX_ESTATE", "MOX_EINVAL", "MOX_ENOMEM",
                   "untouched", "MOX_RANK_GRID", "MOX_TEST_FAIL_RANK", "mox_exchange", "gather first", "wins over the", "mox_sort_result",
                   "accumulator are unchanged", "ranked table is ranked", "rebased to 0", "byte for byte", "first >= N"):
        assert phrase in doc, phrase
    # the order paragraphs of the readers name the ranking
    assert "mox_rank_result" in raw.split("#define MOX_TOP_MAX")[0].split("int mox_sort_result")[1]
    assert "mox_rank_result" in raw.split("int mox_write_result")[0].split("#define MOX_TOP_MAX")[1]


def test_python_mirror_has_the_c_layout(tmp_path):
    """sizeof and every field offset of mox_rank_info, from a probe compiled against the header."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mox_rank_info));']
    for field, _ in mox.RankInfo._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(mox_rank_info, %s));' % (field, field))
    lines += ['  printf("asc %u\\n", MOX_RANK_ASCENDING);', '  printf("max %llu\\n", (unsigned long long)MOX_RANK_MAX_WORDS);',
              "  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(mox.RankInfo) == 80
    for field, _ in mox.RankInfo._fields_:
        assert int(got[field]) == getattr(mox.RankInfo, field).offset, field
    assert int(got["asc"]) == mox.RANK_ASCENDING == 1
    assert int(got["max"]) == mox.RANK_MAX_WORDS == (1 << 32) - 1


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_both_symbols(path):
    raw = ctypes.CDLL(path)
    assert hasattr(raw, "mox_rank_result") and hasattr(raw, "mox_fetch_rows")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_rank_result
    assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(mox.RankInfo)]
    g = L.mox_fetch_rows
    assert g.restype is ctypes.c_int and list(g.argtypes)[:3] == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]


def test_null_arguments_are_einval_and_leave_the_info():
    L = mox.lib()
    info = mox.RankInfo(words=5, tokens=6, max_count=7, digit_passes=8, device_bytes=9)
    assert L.mox_rank_result(None, 0, ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    # unknown flag bits are refused before the engine is looked at (no device is touched: this handle is no engine)
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.mox_rank_result(bogus, 2, ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"flags" in L.mox_last_error()
    assert (info.words, info.tokens, info.max_count, info.digit_passes, info.device_bytes) == (5, 6, 7, 8, 9)
    t = ctypes.POINTER(mox._Table)()
    assert L.mox_fetch_rows(None, 0, 1, ctypes.byref(t)) == mox.MOX_EINVAL and not t
    assert L.mox_fetch_rows(bogus, 0, 1, None) == mox.MOX_EINVAL


def test_python_surface():
    sig = inspect.signature(mox.Engine.rank_result)
    assert list(sig.parameters)[1:] == ["ascending"] and sig.parameters["ascending"].default is False
    assert list(inspect.signature(mox.Engine.fetch_rows).parameters)[1:] == ["first", "n"]
    assert [f for f, _ in mox.RankInfo._fields_] == ["words", "tokens", "max_count", "digit_passes", "device_bytes", "ms", "reserved"]


def test_constants_and_kernels_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_rank.hip")
    t = int(re.search(r"^constexpr int RK_T = (\d+);", src, re.M).group(1))
    steps = int(re.search(r"^constexpr int RK_STEPS = (\d+);", src, re.M).group(1))
    assert re.search(r"^constexpr uint32_t RK_TILE = RK_T \* RK_STEPS;", src, re.M)
    assert re.search(r"^constexpr uint32_t RK_WROWS = 64 \* RK_STEPS;", src, re.M)
    assert t * steps == C.TILE and 64 * steps == C.WAVE_ROWS and t % 64 == 0
    assert int(re.search(r"^constexpr int RK_TOP_T = (\d+);", src, re.M).group(1)) == C.TOP_STEP
    assert C.TOP_MAX == mox.TOP_MAX
    for k in KERNELS:
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
    assert set(re.findall(r"\b(k_rk_\w+)\(", src)) == set(KERNELS)
    # the LDS list of long words only: no atomic, global or not, places a row; and no workgroup waits on another
    assert set(re.findall(r"atomic\w+\(&?(\w+)", src)) == {"s_nbig"}
    assert not re.search(r"\bwhile\b|s_sleep|__threadfence|volatile", src.split("namespace mox_host")[0])
    # the header comment carries the compiler's resource report of every kernel
    report = src.split("#include")[0].split("Resource usage")[1]
    for k in KERNELS:
        assert re.search(r"%s\s+\d+ VGPRs, \d+ SGPRs,\s+\d+ B LDS, no scratch, no spills" % k, report), k
    op_objects("rank", hc=False)  # one object, with KERNEL_FLAGS, once in each of the three libraries
    host = _read("map-oxidize_amd", "csrc", "mox_host.h")
    assert "DevBuf r_tab[2][3], r_tmp;" in host and "bool ranked = false;" in host  # (freed: test_result_buffers.py)


def test_ranked_is_treated_wherever_sorted_is_written():
    """Every writer of Res::sorted has Res::ranked next to it, and the three implicit sorts skip a ranked result."""
    for name, writers in (("mox_engine.hip", 1), ("mox_multi.hip", 2), ("mox_accum.hip", 1), ("mox_bsort.hip", 1)):
        src = _read("map-oxidize_amd", "csrc", name)
        pairs = re.findall(r"^\s*(?:e->res|res|r)\.sorted = [^;]+;\n\s*(?:e->res|res|r)\.ranked = ", src, re.M)
        assert len(pairs) == writers == len(re.findall(r"^\s*(?:e->res|res|r)\.sorted = ", src, re.M)), name
    cond = "(e->flags & MOX_F_SORT_BYTES) && !e->res.sorted && !e->res.ranked"
    assert _read("map-oxidize_amd", "csrc", "mox_engine.hip").count(cond) == 1  # mox_fetch_table and mox_fetch_rows share it
    assert _read("map-oxidize_amd", "csrc", "mox_text.hip").count(cond) == 1
    for name in ("mox_engine.hip", "mox_text.hip"):
        assert "MOX_F_SORT_BYTES) && !e->res.sorted)" not in _read("map-oxidize_amd", "csrc", name), name


def test_expected_on_hand_written_cases():
    items = [(b"the", 9), (b"un", 2), (b"zero", 0), (b"u", 9), (b"max", C.U64), (b"b", 2), (b"z2", 0), (b"a", 2)]
    assert C.expected(items) == [(b"max", C.U64), (b"the", 9), (b"u", 9), (b"un", 2), (b"b", 2), (b"a", 2), (b"zero", 0), (b"z2", 0)]
    assert C.expected(items, ascending=True) == [(b"zero", 0), (b"z2", 0), (b"un", 2), (b"b", 2), (b"a", 2), (b"the", 9), (b"u", 9),
                                                 (b"max", C.U64)]
    # ties keep their order in both directions, so ascending is not descending reversed ...
    assert C.expected(items, ascending=True) != C.expected(items)[::-1]
    # ... and ranking a ranking never moves a tie: ascending after descending is ascending on the original
    assert C.expected(C.expected(items), ascending=True) == C.expected(items, ascending=True)
    assert C.expected([]) == [] and C.expected([(b"x", 0)]) == [(b"x", 0)]
    # the numpy form agrees with the list form
    import numpy as np
    cnt = np.array([c for _, c in items], dtype=np.uint64)
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(w) for w, _ in items])
    for asc in (False, True):
        rc, ro, rb = C.ranked_arrays(cnt, offs, b"".join(w for w, _ in items), asc)
        want = C.expected(items, asc)
        assert rc.tolist() == [c for _, c in want] and rb == b"".join(w for w, _ in want)
        assert ro.tolist() == [sum(len(w) for w, _ in want[:i]) for i in range(len(want) + 1)]
    assert C.expected([(b"b", 5), (b"a", 5)]) == [(b"b", 5), (b"a", 5)]
    # sort_result, then rank_result: count descending, then bytewise
    assert C.expected(sorted(items)) == sorted(items, key=lambda wc: (-wc[1], wc[0]))
    assert C.info_of(items) == {"words": 8, "tokens": (24 + C.U64) & C.U64, "max_count": C.U64, "digit_passes": 8}
    assert C.info_of([]) == {"words": 0, "tokens": 0, "max_count": 0, "digit_passes": 0}
    assert C.info_of([(b"x", 300)]) == {"words": 1, "tokens": 300, "max_count": 300, "digit_passes": 0}
    assert [C.passes_of(m) for m, _ in C.DIGIT_EDGES] == [p for _, p in C.DIGIT_EDGES] == [0, 1, 1, 2, 2, 3, 5, 8, 8]


def test_case_tables_have_their_shapes():
    assert C.TABLE_NS == (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
    tiles = (C.STRIDE_N + C.TILE - 1) // C.TILE
    assert tiles == 3 * C.STRIDE_GRID + 1 and C.STRIDE_N % C.TILE == 1
    z = C.zipf_counts(C.ZIPF_N, 5)
    assert len(z) == 200000 and C.passes_of(max(z)) == 3 and min(z) >= 1 and len(set(z)) < len(z) // 10
    for values in ((7, 300), (1, 2, 70000)):
        s = C.spread_counts(3 * C.TILE + 100, values, 9)
        assert set(s) == set(values) and C.straddles([(b"", c) for c in s], values)
    for m, p in C.DIGIT_EDGES:
        c = C.digit_edge_counts(m)
        assert max(c) == m and len(c) == 300 and (m == 0 or 0 in c)
    b7 = C.byte7_only()
    assert len({c & ((1 << 56) - 1) for c in b7}) == 1 and len({c >> 56 for c in b7}) > 100
    b0 = C.byte0_only()
    assert len({c >> 8 for c in b0}) == 1 and len(set(b0)) > 100 and C.passes_of(max(b0)) == 4
    w, c = C.table(5, [1, 2, 3, 4, 5])
    assert len(set(w)) == 5 == len(c)


def test_cli_documents_the_option():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--by-count"' in src and "mox_rank_result" in src and "mox_sort_result" in src
    assert "--by-count" in src.split("#include")[0]


def test_docs_mention_the_ranking():
    for doc, words in (("README.md", ["mox_rank_result", "mox_fetch_rows", "--by-count"]),
                       ("DESIGN.md", ["Ranking the result", "mox_rank.hip", "k_rk_scatter", "look-back",
                                      "Device ranking against fetch + host sort"]),
                       ("INTEGRATION.md", ["mox_rank_result", "mox_rank_info", "mox_fetch_rows"]),
                       (os.path.join("tools", "README.md"), ["rank_timing.py"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
