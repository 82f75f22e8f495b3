"""CPU: the surface of the device text rendering (include/mox.h
mox_write_result / mox_result_text / mox_text_free / mox_run_file, the Python
mirror) and the case tables of test_gpu_result_text.py.  No GPU code runs
here."""
import ctypes
import os
import re

import mox
from conftest import ROOT
from srcpins import _read, op_objects
import text_cases as C


def test_header_declares_the_four_symbols():
    src = _read("include", "mox.h")
    assert re.search(r"^int mox_write_result\(mox_engine\* e, const char\* path\);", src, re.M)
    assert re.search(r"^int mox_result_text\(mox_engine\* e, uint8_t\*\* text, uint64_t\* len\);", src, re.M)
    assert re.search(r"^void mox_text_free\(uint8_t\* text\);", src, re.M)
    assert re.search(r"^int mox_run_file\(mox_engine\* e, const char\* path\);", src, re.M)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", src, re.M)  # additive: the version stays
    assert mox.lib().mox_abi_version() == 4


def test_library_exports_the_symbols_with_their_signatures():
    raw = ctypes.CDLL(mox.LIB_PATH)
    for name in ("mox_write_result", "mox_result_text", "mox_text_free", "mox_run_file"):
        assert hasattr(raw, name), name
        for path in (mox.CHECK_LIB_PATH, mox.HC_LIB_PATH):  # the check builds link the same kernels
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    L = mox.lib()
    VP, P = ctypes.c_void_p, ctypes.POINTER
    assert L.mox_write_result.restype is ctypes.c_int and list(L.mox_write_result.argtypes) == [VP, ctypes.c_char_p]
    assert L.mox_run_file.restype is ctypes.c_int and list(L.mox_run_file.argtypes) == [VP, ctypes.c_char_p]
    assert L.mox_result_text.restype is ctypes.c_int
    assert list(L.mox_result_text.argtypes) == [VP, P(P(ctypes.c_uint8)), P(ctypes.c_uint64)]
    assert L.mox_text_free.restype is None and list(L.mox_text_free.argtypes) == [P(ctypes.c_uint8)]


def test_python_mirror_has_the_three_methods():
    for name in ("write_result", "result_text", "run_file"):
        assert callable(getattr(mox.Engine, name))


def test_null_arguments_are_einval():
    L = mox.lib()
    p, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(7)
    assert L.mox_write_result(None, b"/nonexistent/x") == mox.MOX_EINVAL
    assert L.mox_run_file(None, b"/nonexistent/x") == mox.MOX_EINVAL
    assert L.mox_result_text(None, ctypes.byref(p), ctypes.byref(n)) == mox.MOX_EINVAL
    assert not p
    L.mox_text_free(p)  # NULL is fine to free


def test_constants_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_text.hip")
    assert int(re.search(r"^constexpr uint64_t TX_TILE = (\d+);", src, re.M).group(1)) == C.TILE
    assert int(re.search(r"^constexpr uint32_t TX_LDS = (\d+);", src, re.M).group(1)) == C.LDS
    t = int(re.search(r"^constexpr int TX_T = (\d+);", src, re.M).group(1))
    per = int(re.search(r"^constexpr int TX_PER = (\d+);", src, re.M).group(1))
    assert t * per == C.TILE
    assert int(re.search(r"^constexpr uint64_t TX_SLICE_MIN = (\d+);", src, re.M).group(1)) == 256
    assert C.EDGE_NS == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
    assert all(S >= 256 and S % 16 == 0 for S in C.SLICES)  # the engine takes them as they are


def test_makefile_links_the_kernels_into_every_library():
    for op in ("text", "topk"):
        op_objects(op, hc=False)


def test_expected_is_the_old_writers_format():
    assert C.expected([(b"the", 27), ("żółć".encode(), 1), (b"x", C.U64), (b"z", 0)]) == \
        b"the 27\n" + "żółć".encode() + b" 1\nx 18446744073709551615\nz 0\n"
    assert C.expected([]) == b""


def test_case_tables_have_their_shapes():
    w, c = C.distinct(5000, 1)
    assert len(set(w)) == 5000 and {len(b"%d" % x) for x in c} == set(range(1, 21)) and max(c) <= C.U64
    w, c = C.digit_edges()
    assert w == sorted(w) and len(set(w)) == len(w) == len(c)
    for d in range(1, 20):
        assert 10 ** (d - 1) in c[:41] and 10 ** d - 1 in c[:41]
    assert 10 ** 19 in c[:41] and c[:41].count(C.U64) == 2 and len(c[:41]) == 41
    assert C.digit_pairs(c[41:]) == {(a, b) for a in range(1, 21) for b in range(1, 21)}
    assert all(1 <= x <= C.U64 for x in c)
    w, c = C.word_shapes()
    assert len(set(w)) == len(w) == 3000 == len(c)
    lens = {len(x) for x in w}
    assert set(range(1, 41)) <= lens and max(lens) == C.BIG_LEN and sum(len(x) > 16 for x in w) > 30
    assert sum(len(x) > 64 for x in w) >= 20 and sum(any(b > 127 for b in x) for x in w) >= 5
    s = sorted(w)
    i = next(k for k, x in enumerate(s) if len(x) == C.BIG_LEN)
    assert s[i - 1] == b"L" and s[i + 1] == b"M"  # a 1-byte word on either side in bytewise order
    assert {len(b"%d" % x) for x in c} == set(range(1, 21))
    w, c, lens = C.lds_edge_tiles()
    assert w == sorted(w) and len(set(w)) == len(w) == 3 * C.TILE + 1
    assert C.tile_text_lengths(list(zip(w, c))) == lens == [C.LDS - 1, C.LDS, C.LDS + 1, 5]


def test_slice_classes_on_a_known_text():
    lines = C.lines_of([(b"ab", 5), (b"c", 123), (b"defg", 7)])  # "ab 5\n" "c 123\n" "defg 7\n": 18 bytes
    assert len(C.expected([(b"ab", 5), (b"c", 123), (b"defg", 7)])) == 18
    # edges 1..17: b _ 5 \n | c _ 1 2 3 \n | d e f g _ 7 \n
    assert C.slice_classes(lines, 1) == {"start": 2, "word": 4, "space": 3, "digits": 5, "newline": 3}
    assert C.slice_classes(lines, 18) == dict.fromkeys(C.CLASSES, 0)
    big = C.lines_of([(b"x" * 100, 1)])
    assert C.slices_inside_a_word(big, 16) == 6 and C.slices_inside_a_word(big, 100) == 1
    assert C.slices_inside_a_word(big, 101) == 0 and C.slices_inside_a_word(lines, 2) == 2  # "ab", "ef"


def test_slice_sizes_hit_every_class_on_the_mixed_text():
    """The slice tests render mixed() in bytewise order (after sort_result), so
    the text here is the text there."""
    w, c = C.mixed()
    items = sorted(zip(w, c))
    lines = C.lines_of(items)
    for S in C.SLICES:
        cls = C.slice_classes(lines, S)
        assert all(cls[k] > 0 for k in C.CLASSES), (S, cls)
        assert any(len(x) + len(t) > S for x, t in lines)      # a line longer than a slice
        assert C.slices_inside_a_word(lines, S) > 0            # a slice wholly inside one word
