"""CPU: the surface of the device re-keying (include/mox.h mox_rekey_result,
the Python mirror, the command-line option) and the model and case tables of
test_gpu_rekey.py (rekey_cases.py).  No GPU code runs here."""
import ctypes
import inspect
import os
import re
import string
import subprocess

import pytest

import mox
import rekey_cases as C
from conftest import ROOT
from srcpins import _read, code_only, op_objects, struct_fields

KERNELS = ("k_rekey_count", "k_rekey_scan", "k_rekey_pack")


def test_header_declares_the_rekey():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_REKEY_TRIM_ASCII_PUNCT 0x1u", "#define MOX_REKEY_PUNCT_LO 0xFC00FFFE00000000ull",
              "#define MOX_REKEY_PUNCT_HI 0x78000001F8000001ull"):
        assert d in src, d
    assert "int mox_rekey_result(mox_engine* e, const mox_rekey* k, mox_rekey_info* info );" in src
    assert struct_fields(src, "mox_rekey") == [
        ("uint64_t", "trim_set[2]"), ("uint64_t", "max_chars"), ("uint32_t", "flags"), ("uint32_t", "pad"), ("uint64_t", "reserved[4]")]
    assert struct_fields(src, "mox_rekey_info") == [
        ("uint64_t", "words_in"), ("uint64_t", "words_out"), ("uint64_t", "words_changed"), ("uint64_t", "words_dropped"),
        ("uint64_t", "tokens_in"), ("uint64_t", "tokens_out"), ("uint64_t", "tokens_dropped"), ("uint64_t", "bytes_out"),
        ("uint64_t", "device_bytes"), ("double", "ms"), ("uint64_t", "reserved[4]")]
    # the section follows the ranking's and the contract is written down next to the declarations
    head = "re-keying the device-resident result"
    assert raw.index("ranking the device-resident result by count") < raw.index("int mox_fetch_rows") < raw.index(head) \
        < raw.index("int mox_get_stats")
    doc = raw.split(head)[1].split("mox_get_stats")[0]
    for phrase in ("Bytes >= 128", "never cut", "is_ascii_punctuation", "string.punctuation", "Inner punctuation stays",
                   "(b & 0xC0) != 0x80", "(K+1)-th character start", "Continuation bytes at the very front", "No", "second trim",
                   '"a.b.c" with K = 2 gives "a."', "tokens_out = tokens_in - tokens_dropped", "count 0 stays present",
                   "mox_reduce_pairs gives over the windowed rows", "engine order", "mox_exchange may start from it",
                   "folded state is", "accumulator is untouched", "commutes with sums", "un-re-keyed", "words_changed == 0",
                   "idempotent", "empty", "member 0", "MOX_ESTATE", "MOX_EINVAL", "MOX_ENOMEM", "untouched", "no result",
                   "accumulator is intact", "MOX_REKEY_GRID", "MOX_TEST_FAIL_REKEY", "mox_exchange_host", "100,000"):
        assert phrase in doc, phrase


def test_python_mirrors_have_the_c_layout(tmp_path):
    """sizeof and every field offset of mox_rekey and mox_rekey_info, from a probe compiled against the header."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {",
             '  printf("size_k %zu\\n", sizeof(mox_rekey));', '  printf("size_i %zu\\n", sizeof(mox_rekey_info));']
    for field, _ in mox.Rekey._fields_:
        lines.append('  printf("k.%s %%zu\\n", offsetof(mox_rekey, %s));' % (field, field))
    for field, _ in mox.RekeyInfo._fields_:
        lines.append('  printf("i.%s %%zu\\n", offsetof(mox_rekey_info, %s));' % (field, field))
    lines += ['  printf("flag %u\\n", MOX_REKEY_TRIM_ASCII_PUNCT);',
              '  printf("lo %llu\\n", (unsigned long long)MOX_REKEY_PUNCT_LO);', '  printf("hi %llu\\n", (unsigned long long)MOX_REKEY_PUNCT_HI);',
              "  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size_k"]) == ctypes.sizeof(mox.Rekey) == 64
    assert int(got["size_i"]) == ctypes.sizeof(mox.RekeyInfo) == 112
    for field, _ in mox.Rekey._fields_:
        assert int(got["k." + field]) == getattr(mox.Rekey, field).offset, field
    for field, _ in mox.RekeyInfo._fields_:
        assert int(got["i." + field]) == getattr(mox.RekeyInfo, field).offset, field
    assert int(got["flag"]) == mox.REKEY_TRIM_ASCII_PUNCT == 1
    assert (int(got["lo"]), int(got["hi"])) == mox.ASCII_PUNCT


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_the_symbol(path):
    raw = ctypes.CDLL(path)
    assert hasattr(raw, "mox_rekey_result")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_rekey_result
    assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, ctypes.POINTER(mox.Rekey), ctypes.POINTER(mox.RekeyInfo)]


def test_the_masks_are_string_punctuation():
    got = bytes(b for b in range(128) if (mox.ASCII_PUNCT[b >> 6] >> (b & 63)) & 1)
    assert got == bytes(sorted(string.punctuation.encode())) and len(got) == 32
    assert C.masks_of(string.punctuation.encode()) == mox.ASCII_PUNCT == C.PUNCT_MASKS
    # Rust's char::is_ascii_punctuation: the four ranges of its documentation
    assert got == bytes(list(range(0x21, 0x30)) + list(range(0x3A, 0x41)) + list(range(0x5B, 0x61)) + list(range(0x7B, 0x7F)))


def test_bad_arguments_are_einval_and_leave_the_info():
    L = mox.lib()
    info = mox.RekeyInfo(words_in=5, words_out=6, tokens_in=7)
    k = mox.Rekey()
    assert L.mox_rekey_result(None, ctypes.byref(k), ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    # the spec is refused before the engine is looked at (no device is touched: this handle is no engine)
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.mox_rekey_result(bogus, None, ctypes.byref(info)) == mox.MOX_EINVAL
    assert L.mox_rekey_result(bogus, ctypes.byref(mox.Rekey(flags=2)), ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"flags" in L.mox_last_error()
    assert L.mox_rekey_result(bogus, ctypes.byref(mox.Rekey(pad=1)), ctypes.byref(info)) == mox.MOX_EINVAL
    bad = mox.Rekey()
    bad.reserved[2] = 1
    assert L.mox_rekey_result(bogus, ctypes.byref(bad), ctypes.byref(info)) == mox.MOX_EINVAL
    assert (info.words_in, info.words_out, info.tokens_in) == (5, 6, 7)


def test_python_surface():
    sig = inspect.signature(mox.Engine.rekey_result)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("trim", b""), ("punct", False), ("max_chars", 0)]
    assert [f for f, _ in mox.Rekey._fields_] == ["trim_set", "max_chars", "flags", "pad", "reserved"]
    assert [f for f, _ in mox.RekeyInfo._fields_] == ["words_in", "words_out", "words_changed", "words_dropped", "tokens_in",
                                                      "tokens_out", "tokens_dropped", "bytes_out", "device_bytes", "ms", "reserved"]
    assert tuple(f for f, _ in mox.RekeyInfo._fields_[:8]) == C.INFO_KEYS
    # a byte >= 128 in trim is refused before the engine is touched
    e = mox.Engine.__new__(mox.Engine)
    e._h = None
    with pytest.raises(ValueError):
        e.rekey_result(trim="é".encode())


def test_constants_and_kernels_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_rekey.hip")
    t = int(re.search(r"^constexpr int RQ_T = (\d+);", src, re.M).group(1))
    per = int(re.search(r"^constexpr int RQ_PER = (\d+);", src, re.M).group(1))
    assert re.search(r"^constexpr uint32_t RQ_TILE = RQ_T \* RQ_PER;", src, re.M)
    assert t * per == C.TILE and t % 64 == 0
    assert 'static_assert(RQ_TILE == %d, "tests/rekey_cases.py TILE");' % C.TILE in src
    assert int(re.search(r"^constexpr uint32_t RQ_COOP = (\d+);", src, re.M).group(1)) == C.COOP
    for k in KERNELS:
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
    assert set(re.findall(r"\b(k_rekey_\w+)\(", src)) == set(KERNELS)
    # the LDS list of long words only: no atomic, global or not, places a record; and no workgroup waits on another
    assert set(re.findall(r"atomic\w+\(&?(\w+)", src)) == {"s_nbig"}
    assert not re.search(r"\bwhile\b|s_sleep|__threadfence|volatile", src.split('extern "C" int mox_rekey_result(')[0].split("#include", 1)[1])
    assert "fnv_finish(h)" in src and "reduce_received(" in src and "k_reduce_z" in src
    # the header comment carries the compiler's resource report of every kernel, the slack argument and the serial walk
    head = src.split("#include")[0]
    report = head.split("Resource usage")[1]
    for k in KERNELS:
        assert re.search(r"%s\s+\d+ VGPRs,\s+\d+ SGPRs,\s+\d+ B LDS, no scratch, no spills" % k, report), k
    for phrase in ("slack contract", "never reads before the word's first", "100,000 steps", "mox_accum.hip is untouched"):
        assert phrase in re.sub(r"\n// ?", " ", head), phrase
    op_objects("rekey", hc=True)  # mox_rekey_hc.o (HC_FLAGS) in libmox_hc.so, mox_rekey.o in the two others
    assert "DevBuf q_tc;" in _read("map-oxidize_amd", "csrc", "mox_host.h")  # (freed: test_result_buffers.py)


def test_model_on_hand_written_cases():
    P = set(C.PUNCT)
    w = C.window
    assert [w(x, P) for x in (b"the", b"the,", b"(the)", b"the.", b"don't", b"a.b", b"...", b"", b"'tis'")] == \
        [b"the", b"the", b"the", b"the", b"don't", b"a.b", b"", b"", b"tis"]
    assert w(b"xxaxbxx", {ord("x")}) == b"axb" and w(b"xxxx", {ord("x")}) == b"" and w(b"ab", set()) == b"ab"
    # bytes >= 128 are never stripped: a UTF-8 sequence is never cut
    assert w("«x»".encode(), P) == "«x»".encode() and w("Σ.".encode(), P) == "Σ".encode()
    assert w("Привет,".encode(), P) == "Привет".encode() and w(b"\xa1!", P) == b"\xa1"
    # the cap: characters, not bytes; no second trim; leading continuation bytes are kept and are no character
    assert w(b"a.b.c", P, 2) == b"a." and w(b"(abc)", P, 2) == b"ab" and w(b"abc", P, 3) == b"abc" == w(b"abc", P, 9)
    assert w("日本語".encode(), P, 1) == "日".encode() and w("\U0001d11ez".encode(), P, 1) == "\U0001d11e".encode()
    assert w("éa".encode(), P, 1) == "é".encode() and w("日本語".encode(), P, 2) == "日本".encode()
    assert w(b"\x80\x80ab", P, 1) == b"\x80\x80a" and w(b"\x80" * 20, P, 1) == b"\x80" * 20
    assert w(b"\xbf\x80" + "日本".encode(), P, 1) == b"\xbf\x80" + "日".encode()
    # expected(): merge, drop, wrap, zero counts, the info
    items = [(b"the", 10), (b"the,", 20), (b"...", 4), (b"x" * 17 + b"!", 0), (b"big", C.U64), (b"(big)", 2)]
    table, rows, info = C.expected(items, punct=True)
    assert table == [(b"the", 30), (b"x" * 17, 0), (b"big", 1)]
    assert rows == [(b"the", 10), (b"the", 20), (b"x" * 17, 0), (b"big", C.U64), (b"big", 2)]
    assert info == {"words_in": 6, "words_out": 3, "words_changed": 4, "words_dropped": 1, "tokens_in": 35, "tokens_out": 31,
                    "tokens_dropped": 4, "bytes_out": 23}
    # nothing to do: the items, order included
    same = [(b"b", 1), (b"a", 2)]
    table, rows, info = C.expected(same, punct=True, tokens=99)
    assert table == same == rows and info["words_changed"] == 0 and info["tokens_in"] == 99 == info["tokens_out"]
    assert C.expected(same)[0] == same and C.expected(items, trim=b"", max_chars=0)[2]["words_changed"] == 0
    # idempotent
    once = C.expected(items, punct=True, max_chars=2)[0]
    assert C.expected(once, punct=True, max_chars=2)[2]["words_changed"] == 0
    assert C.expected([(b"ab", 1), (b"ac", 2)], max_chars=1)[0] == [(b"a", 3)]


def test_case_tables_have_their_shapes():
    assert C.EDGE_NS == (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
    assert (C.STRIDE_N + C.TILE - 1) // C.TILE == 5 and C.STRIDE_GRID == 3
    for n in C.EDGE_NS:
        words, counts = C.edge_table(n)
        assert len(set(words)) == n == len(counts)
        _, _, info = C.expected(list(zip(words, counts)), punct=True)
        assert info["words_changed"] == n // 3 and info["words_out"] == n - n // 3 and info["words_dropped"] == 0
    assert any(len(w) > 16 for w in C.edge_table(65)[0])
    words, _ = C.run_table()
    assert len(set(words)) == len(words) == 125
    assert {(len(x) - len(x.lstrip(b"(")), len(x) - len(x.rstrip(b")"))) for x in words} == {(a, b) for a in C.RUNS for b in C.RUNS}
    words, counts = C.phase_table()
    assert C.expected(list(zip(words, counts)), punct=True)[2]["words_out"] == len(words) == 360  # the windows stay distinct
    assert C.phase_cover(sorted(words)) == {(o, lead) for o in range(8) for lead in range(9)}
    words, counts = C.shape_table()
    table, rows, info = C.expected(list(zip(words, counts)), punct=True)
    lens = {len(w) for w, _ in rows}
    assert {15, 16, 17, 100000} <= lens and info["words_dropped"] == 5
    assert sorted(len(w) for w in words if not C.window(w, set(C.PUNCT))) == [1, 16, 17, 300, 100000]
    assert dict(table)[C.BIG_WORD] == sum(c for w, c in rows if w == C.BIG_WORD) and [w for w, _ in rows].count(C.BIG_WORD) == 2
    assert any(b"\x00" in w and len(w) <= 16 for w, _ in rows) and "Σ".encode() in dict(table) and "Привет".encode() in dict(table)
    # long -> short and long -> long at the 16-byte edge
    assert any(len(x) > 16 and len(C.window(x, set(C.PUNCT))) == 16 for x in words)
    words, counts = C.last_is_one_byte()
    assert sorted(words)[-1] == b"~" and sorted(words)[-2] == b"}~"
    words, counts = C.merge_table()
    table = dict(C.expected(list(zip(words, counts)), punct=True)[0])
    assert table[b"the"] == 100 and table[b"a_word_of_20_bytes_x"] == 10 and table[b"zz"] == 0 and table[b"zf"] == 5
    assert table[b"z_long_word_with_count_0"] == 0 and table[b"wrap"] == 1 and table[b"a_long_word_that_wraps"] == 5 and len(table) == 7
    words, counts = C.cap_table()
    items = list(zip(words, counts))
    t1 = dict(C.expected(items, max_chars=1)[0])
    assert {"é".encode(), "日".encode(), "\U0001d11e".encode(), b"a", b"b", b"\x80", b"\x80\x80a", b"\x80" * 20} <= set(t1)
    assert {len(w) for w, _ in C.expected(items, max_chars=16)[0]} >= {16, 20} and C.expected(items, max_chars=17)[2]["words_changed"] > 0
    assert C.expected(items, max_chars=1000)[2]["words_changed"] == 0
    words, counts = C.plain_words(500)
    assert C.expected(list(zip(words, counts)), punct=True)[2]["words_changed"] == 0 and any(len(w) > 16 for w in words)


def test_cli_documents_the_option():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--trim-punct"' in src and "mox_rekey_result" in src and "MOX_REKEY_TRIM_ASCII_PUNCT" in src
    assert "--trim-punct" in src.split("#include")[0]
    # it applies before the filter and the ranking
    body = src.split("int main")[1]
    assert body.index("mox_rekey_result") < body.index("mox_filter_result") < body.index("mox_rank_result")


def test_docs_mention_the_rekey():
    for doc, words in (("README.md", ["mox_rekey_result", "--trim-punct"]),
                       ("DESIGN.md", ["Re-keying the result", "mox_rekey.hip", "k_rekey_pack", "second trim", "Unicode punctuation"]),
                       (os.path.join("tools", "README.md"), ["rekey_timing.py"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
