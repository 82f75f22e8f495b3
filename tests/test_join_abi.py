"""CPU: the surface of the device join (include/mox.h mox_join_total, the
Python mirror, mox.dist.sum_joins, the command-line options) and the case
tables of test_gpu_join.py (join_cases.py).  No GPU code runs here."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import join_cases as C
import lookup_cases as LC
import mox
from conftest import ROOT
from srcpins import _read, code_only, op_objects, struct_fields
from mox import dist

CLI = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")


def test_header_declares_the_join():
    raw = _read("include", "mox.h")
    src = code_only(raw)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", raw, re.M)  # additive: the version stays
    for d in ("#define MOX_JOIN_SEMI 0u", "#define MOX_JOIN_ANTI 1u", "#define MOX_JOIN_COUNTS_RESULT 0u",
              "#define MOX_JOIN_COUNTS_TOTAL 1u", "#define MOX_JOIN_COUNTS_MIN 2u", "#define MOX_JOIN_COUNT_ONLY 0x1u",
              "#define MOX_JOIN_MAX_WORDS 0xFFFFFFFEull"):
        assert d in src, d
    assert "int mox_join_total(mox_engine* e, const mox_join* j, mox_join_info* info );" in src
    assert struct_fields(src, "mox_join") == [
        ("uint32_t", "mode"), ("uint32_t", "counts"), ("uint32_t", "flags"), ("uint32_t", "pad"), ("uint64_t", "reserved[4]")]
    assert struct_fields(src, "mox_join_info") == [
        ("uint64_t", "words_in"), ("uint64_t", "words_total"), ("uint64_t", "words_matched"), ("uint64_t", "words_kept"),
        ("uint64_t", "tokens_in"), ("uint64_t", "tokens_total"), ("uint64_t", "tokens_matched_result"),
        ("uint64_t", "tokens_matched_total"), ("uint64_t", "tokens_min"), ("uint64_t", "tokens_kept"), ("uint64_t", "bytes_kept"),
        ("uint64_t", "tag_mismatch"), ("uint64_t", "device_bytes"), ("double", "ms"), ("uint64_t", "reserved[4]")]
    # the section follows the filter's and the contract is written down next to the declaration
    a = raw.index("filtering the device-resident result")
    b = raw.index("joining the device-resident result against the accumulated total")
    c = raw.index("ranking the device-resident result by count")
    assert a < b < c
    doc = raw[b:c]
    for phrase in ("verbatim", "MOX_ESTATE", "MOX_EINVAL", "MOX_ENOMEM", "untouched", "MOX_JOIN_GRID", "MOX_TEST_FAIL_JOIN",
                   "mox_exchange", "never sorts", "accumulator is untouched", "empty T", "count 0", "ranged owners", "gather first",
                   "hash-owner", "32 to 64 bytes per row", "Ranked state", "wrapping"):
        assert phrase in doc, phrase


def test_python_mirrors_have_the_c_layout(tmp_path):
    """sizeof and every field offset of both structs, from a probe compiled against the header."""
    names = {"mox_join": mox.Join, "mox_join_info": mox.JoinInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mox.h"', "int main(void) {"]
    for cname, py in names.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines.append('  printf("max %llu\\n", (unsigned long long)MOX_JOIN_MAX_WORDS);')
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in names.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(py, field).offset, (cname, field)
    assert ctypes.sizeof(mox.Join) == 48 and ctypes.sizeof(mox.JoinInfo) == 144
    assert (mox.JOIN_SEMI, mox.JOIN_ANTI, mox.JOIN_COUNTS_RESULT, mox.JOIN_COUNTS_TOTAL, mox.JOIN_COUNTS_MIN, mox.JOIN_COUNT_ONLY) == (0, 1, 0, 1, 2, 1)
    assert int(got["max"]) == mox.JOIN_MAX_WORDS == 2 ** 32 - 2


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_the_join(path):
    assert hasattr(ctypes.CDLL(path), "mox_join_total")
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    f = L.mox_join_total
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.POINTER(mox.Join), ctypes.POINTER(mox.JoinInfo)]


def test_null_engine_and_bad_specs_are_einval_and_leave_the_info():
    """Every argument check comes before the engine is looked at: this handle is no engine, and no device is touched."""
    L = mox.lib()
    info = mox.JoinInfo(words_in=5, words_kept=6, tokens_min=7)
    assert L.mox_join_total(None, ctypes.byref(mox.Join()), ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.mox_join_total(bogus, None, ctypes.byref(info)) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()
    for kw in (dict(mode=2), dict(counts=3), dict(flags=2), dict(pad=1), dict(mode=mox.JOIN_ANTI, counts=mox.JOIN_COUNTS_TOTAL),
               dict(mode=mox.JOIN_ANTI, counts=mox.JOIN_COUNTS_MIN)):
        assert L.mox_join_total(bogus, ctypes.byref(mox.Join(**kw)), ctypes.byref(info)) == mox.MOX_EINVAL, kw
    bad = mox.Join()
    bad.reserved[2] = 1
    assert L.mox_join_total(bogus, ctypes.byref(bad), ctypes.byref(info)) == mox.MOX_EINVAL
    assert (info.words_in, info.words_kept, info.tokens_min) == (5, 6, 7)


def test_python_surface_and_argument_errors():
    sig = inspect.signature(mox.Engine.join_total)
    assert list(sig.parameters)[1:] == ["mode", "counts", "count_only"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == ["semi", "result", False]

    class NoCalls:  # a bad string is refused before any C call: nothing of the engine is touched
        def __getattr__(self, name):
            raise AssertionError("the engine was used: %s" % name)

    for kw in (dict(mode="inner"), dict(mode="SEMI"), dict(counts="sum"), dict(mode="anti", counts="max"), dict(mode=0)):
        with pytest.raises(ValueError):
            mox.Engine.join_total(NoCalls(), **kw)


def test_sum_joins():
    a = dict.fromkeys(C.INFO_KEYS, 3)
    a.update(tag_mismatch=1, device_bytes=100, ms=2.5)
    b = dict.fromkeys(C.INFO_KEYS, 4)
    b.update(tag_mismatch=0, device_bytes=70, ms=4.0, tokens_min=C.U64)
    want = dict.fromkeys(C.INFO_KEYS, 7)
    want.update(tag_mismatch=1, device_bytes=100, ms=4.0, tokens_min=2)  # u64 sums wrap; the two others: the largest
    assert dist.sum_joins([a, b]) == want
    assert dist.sum_joins([a]) == a and dist.sum_joins([]) == {}


def test_constants_match_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_join.hip")
    ws = _read("map-oxidize_amd", "csrc", "mox_wordset.h")  # the geometry is the word set's, shared with the lookup
    t = int(re.search(r"^constexpr int WS_T = (\d+);", ws, re.M).group(1))
    per = int(re.search(r"^constexpr int WS_PER = (\d+);", ws, re.M).group(1))
    assert re.search(r"^constexpr uint32_t WS_TILE = WS_T \* WS_PER;", ws, re.M)
    assert t * per == C.TILE == LC.TILE and t % 64 == 0
    assert 'static_assert(WS_TILE == %d, "tests/lookup_cases.py and tests/join_cases.py TILE");' % C.TILE in ws
    for k in ("k_jn_build", "k_jn_stream", "k_jn_apply"):
        assert re.search(r'extern "C" __global__ .* void %s\(' % k, src) and 'q.step("%s")' % k in src, k
        assert re.search(r"^//   %s .*no scratch.*\(\d waves / SIMD\)$" % k, src, re.M), k  # its resource usage is written down
    # the set, the hash and the compare are the lookup's, from one header; the compaction is the filter's own
    assert '#include "mox_wordset.h"' in src and '#include "mox_wordset.h"' in _read("map-oxidize_amd", "csrc", "mox_lookup.hip")
    assert '#include "mox_wordhash.h"' in ws and "lk_hash" in _read("map-oxidize_amd", "csrc", "mox_wordhash.h")
    flt = _read("map-oxidize_amd", "csrc", "mox_filter.hip")
    assert 'extern "C" int mox_join_total(' in flt and "k_fl_" not in re.sub(r"//.*", "", src)  # no second compaction
    for name in ("mox_dev.h", "mox_host.h"):
        assert "mox_join.hip" in _read("map-oxidize_amd", "csrc", name).split("#pragma once")[0], name
    assert "DevBuf j_tmp;" in _read("map-oxidize_amd", "csrc", "mox_host.h")  # (freed: test_result_buffers.py)


def test_the_word_set_is_in_one_place():
    """The lookup and the join hold a policy, their third kernel and the host side: the compare-and-swap
    and every probe loop over the slots are mox_wordset.h's."""
    probe = (r"\batomicCAS\b", r"\bp = 0\b", r"\bslots\[", r"\bslots \+", r"& S\.mask", r"\bs_big\b", r"\blk_hash\b", r"\blk_equal\b")
    ws = re.sub(r"//.*", "", _read("map-oxidize_amd", "csrc", "mox_wordset.h"))
    for pat in probe:
        assert re.search(pat, ws), pat
    assert len(re.findall(r"\batomicCAS\b", ws)) == 1  # one claim
    for name, policy in (("mox_lookup.hip", "LkWords"), ("mox_join.hip", "JnWords")):
        code = re.sub(r"//.*", "", _read("map-oxidize_amd", "csrc", name))
        for pat in probe:
            assert not re.search(pat, code), (name, pat)
        assert code.count("ws_build<%s>(S);" % policy) == 1 and code.count("ws_stream<%s>(T, S);" % policy) == 1, name
        assert "ws_slots(" in code, name  # the one slot rule


def test_makefile_links_the_join():
    op_objects("join", hc=True)  # mox_join_hc.o (KERNEL_FLAGS and HC_FLAGS) in libmox_hc.so, mox_join.o in the two others
    deps = re.search(r"^HOST_DEPS := (.*)$", _read("Makefile"), re.M).group(1)
    assert "mox_wordhash.h" in deps and "mox_wordset.h" in deps


def test_expected_on_hand_written_cases():
    r = [(b"the", 9), (b"ab", 2), (b"new", 1), (b"zero", 5), (b"ab\x00", 4)]
    t = [(b"zero", 0), (b"ab", 7), (b"the", 3), (b"old", 8)]
    kept, info = C.expected(r, t, "semi", "result")
    assert kept == [(b"the", 9), (b"ab", 2), (b"zero", 5)]  # a zero-count total word is held; "ab\0" is not "ab"
    assert info == {"words_in": 5, "words_total": 4, "words_matched": 3, "words_kept": 3, "tokens_in": 21, "tokens_total": 18,
                    "tokens_matched_result": 16, "tokens_matched_total": 10, "tokens_min": 5, "tokens_kept": 16, "bytes_kept": 9}
    kept, info = C.expected(r, t, "anti")
    assert kept == [(b"new", 1), (b"ab\x00", 4)]
    assert (info["words_matched"], info["words_kept"], info["tokens_kept"], info["bytes_kept"], info["tokens_min"]) == (3, 2, 5, 6, 5)
    kept, info = C.expected(r, t, "semi", "total")
    assert kept == [(b"the", 3), (b"ab", 7), (b"zero", 0)] and info["tokens_kept"] == 10  # ... and written as 0
    kept, info = C.expected(r, t, "semi", "min")
    assert kept == [(b"the", 3), (b"ab", 2), (b"zero", 0)] and info["tokens_kept"] == 5 == info["tokens_min"]  # the smaller one, from either side
    # ANTI against an empty T keeps everything, SEMI nothing
    kept, info = C.expected(r, [], "anti")
    assert kept == r and info["words_matched"] == 0 == info["tokens_total"] and info["tokens_kept"] == 21
    assert C.expected(r, [], "semi", "total")[0] == [] and C.expected([], t, "anti") == ([], dict(dict.fromkeys(C.INFO_KEYS, 0), words_total=4, tokens_total=18))
    # u64 sums wrap
    big_r, big_t = [(b"x", C.U64), (b"y", 2)], [(b"x", 5), (b"y", C.U64)]
    info = C.expected(big_r, big_t, "semi", "min")[1]
    assert info["tokens_min"] == 7 and info["tokens_in"] == 1 and info["tokens_matched_total"] == 4
    assert C.expected(big_r, big_t, "semi", "total")[1]["tokens_kept"] == 4
    with pytest.raises(AssertionError):
        C.expected(r, t, "anti", "total")
    with pytest.raises(AssertionError):
        C.expected(r, [(b"a", 1), (b"a", 2)])
    # the two modes partition R
    assert sorted(C.expected(r, t, "semi")[0] + C.expected(r, t, "anti")[0]) == sorted(r)


def test_case_tables_have_their_shapes():
    assert C.TILE == 1024 and C.TABLE_NS == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
    assert C.STRIDE_N == 5 * C.TILE + 1 and C.STRIDE_GRID == 2
    assert (C.STRIDE_N + C.TILE - 1) // C.TILE == 3 * C.STRIDE_GRID  # three strides of T; the set holds more rows than one tile
    for n_r, n_t in ((1, 300), (300, 1), (300, 300), (1025, 300), (C.STRIDE_N, C.STRIDE_N)):
        (rw, rc), (tw, tc) = C.pair(n_r, n_t, 5)
        assert len(set(rw)) == n_r == len(rc) and len(set(tw)) == n_t == len(tc)
        shared = set(rw) & set(tw)
        assert len(shared) == max(1, min(n_r, n_t) // 3)
        r, t = dict(zip(rw, rc)), dict(zip(tw, tc))
        assert all(r[w] != t[w] for w in shared) and min(tc) >= 0
        if len(shared) > 1:
            assert any(r[w] < t[w] for w in shared) and any(r[w] > t[w] for w in shared)
    assert {len(x) for x in C.shape_table()[0]} >= {15, 16, 17, 63, 64, 65, 100000}


@pytest.mark.parametrize("args", [
    ["--not-in", "base.txt", "--also-in", "base.txt"],
    ["--not-in", "base.txt", "--not-in", "other.txt"],
    ["--not-in", "base.txt", "a.txt", "b.txt"],
    ["--also-in", "base.txt", "a.txt", "b.txt"],
    ["--also-in", "base.txt", "--chunk", "4096", "a.txt"],
    ["--not-in", "base.txt", "--chunk", "4096"],
])
def test_cli_usage_errors_give_status_2(tmp_path, args):
    """Refused from the arguments alone: no engine is created and no file is opened."""
    r = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.startswith(b"Usage:") and r.stdout == b""
    assert not (tmp_path / "final_result.txt").exists()


def test_cli_and_docs_mention_the_join():
    src = _read("map-oxidize_amd", "csrc", "meduce_gpu.cpp")
    assert '"--not-in"' in src and '"--also-in"' in src and "mox_join_total" in src
    for doc, words in (("README.md", ["mox_join_total", "--not-in"]),
                       ("DESIGN.md", ["Joining the result against the total", "mox_join.hip", "k_jn_stream",
                                      "Device join against fetch + host join + reduce_pairs", "a dot product of the counts"]),
                       (os.path.join("tools", "README.md"), ["join_timing.py"]),
                       (os.path.join("profiles", "join", "README.md"), ["k_jn_stream"])):
        text = _read(doc)
        for w in words:
            assert w in text, (doc, w)
