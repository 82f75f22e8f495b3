"""CPU: the surface of the device filter (include/mox.h mox_filter_result, the
Python mirror, the command-line options) and the case tables of
test_gpu_filter.py (filter_cases.py).  No GPU code runs here."""
import ctypes
import os
import re
import subprocess

import pytest

import filter_cases as C
import mox
from conftest import ROOT
from srcpins import _read, code_only, op_objects, struct_fields


def test_header_declares_the_filter():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_FILTER_PREFIX_MAX 16", "#define MOX_FILTER_WORDS_DROP 0u", "#define MOX_FILTER_WORDS_KEEP 1u",
              "#define MOX_FILTER_COUNT_ONLY 0x1u"):
        assert d in src, d
    assert "int mox_filter_result(mox_engine* e, const mox_filter* f, mox_filter_info* info );" in src
    assert struct_fields(src, "mox_filter") == [
        ("uint64_t", "min_count"), ("uint64_t", "max_count"), ("uint64_t", "min_len"), ("uint64_t", "max_len"),
        ("const uint8_t*", "prefix"), ("uint64_t", "prefix_len"), ("const uint8_t*", "words"), ("const uint64_t*", "word_offs"),
        ("uint64_t", "n_words"), ("uint32_t", "words_mode"), ("uint32_t", "flags"), ("uint64_t", "reserved[4]")]
    assert struct_fields(src, "mox_filter_info") == [
        ("uint64_t", "words_in"), ("uint64_t", "words_kept"), ("uint64_t", "tokens_in"), ("uint64_t", "tokens_kept"),
        ("uint64_t", "bytes_kept"), ("uint64_t", "list_found"), ("uint64_t", "device_bytes"), ("double", "ms"),
        ("uint64_t", "reserved[4]")]
    # the section follows the lookup's and the contract is written down next to the declaration
    assert raw.index("looking words up in the device-resident result") < raw.index("filtering the device-resident result")
    doc = raw.split("filtering the device-resident result")[1].split("mox_get_stats")[0]
    for phrase in ("verbatim", "MOX_ESTATE", "MOX_EINVAL", "MOX_ENOMEM", "untouched", "MOX_FILTER_GRID", "MOX_TEST_FAIL_FILTER",
                   "mox_exchange", "cannot be selected alone", "shorter than the prefix", "never sorts", "un-exchanged",
                   "accumulator is untouched", "conjunction"):
        assert phrase in doc, phrase


def test_python_mirrors_have_the_c_layout(tmp_path):
    """sizeof and every field offset of both structs, from a probe compiled against the header."""
    names = {"mox_filter": mox.Filter, "mox_filter_info": mox.FilterInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {"]
    for cname, py in names.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in names.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(py, field).offset, (cname, field)
    assert ctypes.sizeof(mox.Filter) == 112 and ctypes.sizeof(mox.FilterInfo) == 96
    assert (mox.FILTER_PREFIX_MAX, mox.FILTER_WORDS_DROP, mox.FILTER_WORDS_KEEP, mox.FILTER_COUNT_ONLY) == (16, 0, 1, 1)


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_the_filter(path):
    assert hasattr(ctypes.CDLL(path), "mox_filter_result")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_filter_result
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.POINTER(mox.Filter), ctypes.POINTER(mox.FilterInfo)]


def test_null_engine_and_null_filter_are_einval_and_leave_the_info():
    L = mox.lib()
    f = mox.Filter()
    info = mox.FilterInfo(words_in=5, words_kept=6, tokens_in=7, tokens_kept=8, bytes_kept=9, list_found=10)
    assert L.mox_filter_result(None, ctypes.byref(f), ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    # a NULL filter is refused before the engine is looked at (no device is touched: this handle is no engine)
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.mox_filter_result(bogus, None, ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    assert (info.words_in, info.words_kept, info.tokens_in, info.tokens_kept, info.bytes_kept, info.list_found) == (5, 6, 7, 8, 9, 10)


def test_python_surface():
    assert callable(mox.Engine.filter_result) and callable(mox.Engine.filter_result_packed)
    import inspect
    sig = inspect.signature(mox.Engine.filter_result)
    assert list(sig.parameters)[1:] == ["min_count", "max_count", "min_len", "max_len", "prefix", "drop", "keep", "count_only"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [0, None, 0, None, b"", None, None, False]


def test_constants_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_filter.hip")
    t = int(re.search(r"^constexpr int FL_T = (\d+);", src, re.M).group(1))
    per = int(re.search(r"^constexpr int FL_PER = (\d+);", src, re.M).group(1))
    assert re.search(r"^constexpr uint32_t FL_TILE = FL_T \* FL_PER;", src, re.M)
    assert t * per == C.TILE and t % 64 == 0
    hdr = _read("include", "mox.h")
    assert int(re.search(r"^#define MOX_FILTER_PREFIX_MAX (\d+)", hdr, re.M).group(1)) == C.PREFIX_MAX == mox.FILTER_PREFIX_MAX
    assert C.LOOKUP_MAX == mox.LOOKUP_MAX
    for k in ("k_fl_mark", "k_fl_count", "k_fl_scan", "k_fl_emit"):
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
    # the LDS list of long words and list_found only: no global atomic places a row
    assert set(re.findall(r"atomicAdd\(&?(\w+)", src)) == {"s_nf", "found", "s_nbig"}
    op_objects("filter", hc=False)  # no mox_filter_hc.o: the plain object in all three libraries


def test_expected_on_hand_written_cases():
    items = [(b"the", 9), (b"un", 2), (b"undo", 1), (b"zero", 0), (b"u", 4), (b"unlikely", 3), (b"a\x00b", 2)]
    all_info = {"words_in": 7, "words_kept": 7, "tokens_in": 21, "tokens_kept": 21, "bytes_kept": 25, "list_found": 0}
    assert C.expected(items) == (items, all_info)
    kept, info = C.expected(items, min_count=2)
    assert kept == [(b"the", 9), (b"un", 2), (b"u", 4), (b"unlikely", 3), (b"a\x00b", 2)]
    assert info == {"words_in": 7, "words_kept": 5, "tokens_in": 21, "tokens_kept": 20, "bytes_kept": 17, "list_found": 0}
    assert C.expected(items, min_count=1, max_count=1)[0] == [(b"undo", 1)]  # the hapax
    assert C.expected(items, min_count=3, max_count=2)[0] == []
    assert C.expected(items, max_count=0)[0] == items and C.expected(items, max_len=0)[0] == items  # 0: no upper bound
    assert C.expected(items, min_count=1)[0] == [x for x in items if x[0] != b"zero"]
    assert C.expected(items, min_len=2, max_len=3)[0] == [(b"the", 9), (b"un", 2), (b"a\x00b", 2)]
    assert C.expected(items, prefix=b"un")[0] == [(b"un", 2), (b"undo", 1), (b"unlikely", 3)]
    assert C.expected(items, prefix=b"und")[0] == [(b"undo", 1)]  # "un" and "u" are shorter than the prefix
    assert C.expected(items, prefix=b"a\x00")[0] == [(b"a\x00b", 2)]
    kept, info = C.expected(items, drop=[b"the", b"a", b"the", b"u"])
    assert kept == [(b"un", 2), (b"undo", 1), (b"zero", 0), (b"unlikely", 3), (b"a\x00b", 2)]
    assert info["list_found"] == 2 and info["tokens_kept"] == 8 and info["bytes_kept"] == 21
    kept, info = C.expected(items, keep=[b"zero", b"The", b"u"])
    assert kept == [(b"zero", 0), (b"u", 4)] and info["list_found"] == 2
    assert C.expected(items, keep=[])[0] == [] and C.expected(items, drop=[])[0] == items
    kept, info = C.expected(items, min_count=2, min_len=2, prefix=b"u", drop=[b"un"])
    assert kept == [(b"unlikely", 3)] and info["list_found"] == 1  # found in the table, whatever the other terms say
    assert C.expected([], min_count=1) == ([], dict.fromkeys(C.INFO_KEYS, 0))
    big = [(b"x", C.U64), (b"y", 2)]
    assert C.expected(big)[1]["tokens_kept"] == 1  # u64 sums wrap
    with pytest.raises(AssertionError):
        C.expected(items, drop=[b"a"], keep=[b"b"])
    # twice == the conjunction
    once = C.expected(items, min_count=2, prefix=b"u")[0]
    assert C.expected(C.expected(items, min_count=2)[0], prefix=b"u")[0] == once == [(b"un", 2), (b"u", 4), (b"unlikely", 3)]


def test_case_tables_have_their_shapes():
    assert C.TABLE_NS == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
    tiles = (C.STRIDE_N + C.TILE - 1) // C.TILE
    assert tiles >= 3 * C.STRIDE_GRID and C.STRIDE_N % C.TILE == 1
    w, c = C.random_words(5000, 3)
    assert len(set(w)) == 5000 == len(c) and 0 in c and max(c) == 40
    assert sum(x.startswith(b"un") for x in w) > 50 and {len(x) for x in w} >= set(range(3, 31))
    for n in C.LIST_NS:
        lw = C.list_words(w, n, n)
        assert len(lw) == n and any(x in set(w) for x in lw)
        if n > 1:
            assert any(x not in set(w) for x in lw) and len(set(lw)) < n
    sw, _ = C.shape_table()
    lens = {len(x) for x in sw}
    assert lens >= {15, 16, 17, 63, 64, 65, 100000}


def test_cli_documents_the_options():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--min-count"' in src and '"--stop"' in src and "mox_filter_result" in src


def test_docs_mention_the_filter():
    for doc, words in (("README.md", ["mox_filter_result", "--stop"]),
                       ("DESIGN.md", ["Filtering the result", "mox_filter.hip", "k_fl_emit"]),
                       ("INTEGRATION.md", ["mox_filter_result", "mox_filter_info"]),
                       (os.path.join("tools", "README.md"), ["filter_timing.py"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
