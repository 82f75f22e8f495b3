"""CPU: the accumulator's C ABI (include/mox.h: mox_accumulate,
mox_accumulate_file, mox_accumulate_reset, mox_accumulate_info), its Python
surface, and the models the GPU tests rely on (accum_cases.py): the
classification rule, the shapes of the case tables and the chunk-cut rule."""
import ctypes
import os
import re

import pytest

import accum_cases as C
import mox
from conftest import ROOT
from srcpins import code_only

FUNCS = ["mox_accumulate", "mox_accumulate_file", "mox_accumulate_reset", "mox_accumulate_info"]


def header():
    return open(os.path.join(ROOT, "include", "mox.h")).read()


def test_header_declares_the_accumulator():
    src = code_only(header())
    assert "#define MOX_ABI_VERSION 4" in src
    assert "int mox_accumulate(mox_engine* e);" in src
    assert "int mox_accumulate_file(mox_engine* e, const char* path, uint64_t chunk_bytes);" in src
    assert "int mox_accumulate_reset(mox_engine* e);" in src
    assert "int mox_accumulate_info(const mox_engine* e, mox_accum_info* out);" in src
    m = re.search(r"typedef struct mox_accum_info \{(.*?)\} mox_accum_info;", src)
    assert m, "mox_accum_info"
    fields = re.findall(r"uint64_t ([a-z_, ]+);", m.group(1))
    assert [f.strip() for grp in fields for f in grp.split(",")] == ["passes", "words", "tokens", "device_bytes"]
    assert ctypes.sizeof(mox.AccumInfo) == 32
    assert [f for f, _ in mox.AccumInfo._fields_] == ["passes", "words", "tokens", "device_bytes"]
    # the contract is written down next to the declarations
    for phrase in ("MOX_ESTATE", "MOX_TEST_FAIL_ACCUM", "ASCII whitespace"):
        assert phrase in header().split("accumulating results on the device")[1].split("mox_get_stats")[0]


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_every_library_exports_the_accumulator(path):
    L = mox.lib(path)
    assert L.mox_abi_version() == 4
    for f in FUNCS:
        fn = getattr(L, f)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert L.mox_accumulate_file.argtypes[2] is ctypes.c_uint64


def test_null_arguments_are_einval():
    L = mox.lib()
    info = mox.AccumInfo()
    assert L.mox_accumulate(None) == mox.MOX_EINVAL
    assert L.mox_accumulate_reset(None) == mox.MOX_EINVAL
    assert L.mox_accumulate_info(None, ctypes.byref(info)) == mox.MOX_EINVAL
    assert L.mox_accumulate_file(None, b"x", 0) == mox.MOX_EINVAL
    assert b"NULL" in L.mox_last_error()


def test_python_surface():
    for m in ("accumulate", "accumulate_file", "accumulate_reset", "accumulate_info"):
        assert callable(getattr(mox.Engine, m))
    assert callable(mox.count_files)


def test_cli_documents_its_inputs():
    src = open(os.path.join(ROOT, "map-oxidize_amd", "csrc", "meduce_gpu.cpp")).read()
    assert '"--chunk"' in src and "mox_accumulate_file" in src


def test_tile_constant_matches_the_packer():
    src = open(os.path.join(ROOT, "map-oxidize_amd", "csrc", "mox_accum.hip")).read()
    t = int(re.search(r"constexpr int AC_T = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int AC_PER = (\d+);", src).group(1))
    assert "AC_TILE = AC_T * AC_PER" in src
    assert t * per == C.TILE


def test_classification_model():
    assert C.is_short(b"a") and C.is_short(C.W16) and C.is_short("日本語".encode())
    assert not C.is_short(b"") and not C.is_short(C.W16 + b"!")
    assert not any(C.is_short(w) for w in C.NUL_WORDS[1:]) and C.is_short(C.NUL_WORDS[0])
    assert not C.is_short(C.BIG_WORD) and b"\x00" not in C.BIG_WORD and len(C.BIG_WORD) == 100000
    assert not C.is_short(b"x" * 16 + b"\x00") and not C.is_short(b"\x00" * 16)
    assert C.is_short(b"\x01" * 16)


def test_edge_tables_shapes():
    assert sorted(a for a, _ in C.EDGE_PAIRS) == sorted(C.EDGE_NS) == sorted(b for _, b in C.EDGE_PAIRS)
    assert {0, 1, 63, 64, 65, C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1} == set(C.EDGE_NS)
    (wa, ca), (wb, cb) = C.edge_tables(2 * C.TILE + 1, C.TILE + 1, "alternate")
    assert len(set(wa)) == len(wa) == len(ca) and len(set(wb)) == len(wb) == len(cb)
    shared = set(wa) & set(wb)
    assert len(shared) == (C.TILE + 2) // 2  # every second word of B
    assert not set(C.edge_tables(65, 64, "disjoint")[0][0]) & set(C.edge_tables(65, 64, "disjoint")[1][0])
    assert set(C.edge_tables(65, 64, "identical")[1][0]) <= set(C.edge_tables(65, 64, "identical")[0][0])
    # short and long rows interleave, and start at every phase of an 8-byte word
    kinds = [C.is_short(w) for w in wa]
    assert any(a and not b for a, b in zip(kinds, kinds[1:])) and any(b and not a for a, b in zip(kinds, kinds[1:]))
    s, l = C.phases(wa)
    assert s == set(range(8)) and l == set(range(8))


def test_shape_tables_shapes():
    (wa, ca), (wb, cb) = C.shape_tables()
    assert len(set(wa)) == len(wa) == len(ca) and len(set(wb)) == len(wb) == len(cb)
    assert {len(w) for w in wa} >= set(range(1, 41)) and C.W16 in wa and C.W16 + b"!" in wa
    assert all(w in wa for w in C.NUL_WORDS) and len(set(C.NUL_WORDS)) == 4
    per_char = {len(ch.encode()) for w in C.UTF8_WORDS for ch in w.decode()}
    assert per_char >= {2, 3, 4}
    for w in (C.BIG_WORD, C.LONG_BOTH, C.SHORT_BOTH):
        assert w in wa and w in wb
    assert C.is_short(C.SHORT_BOTH) and not C.is_short(C.LONG_BOTH)
    assert set(wb) - set(wa) and set(wa) - set(wb)
    s, l = C.phases(wa)
    assert s == set(range(8)) and l == set(range(8))
    for t in (C.LAST1, C.LAST1_OTHER):
        assert len(max(t[0])) == 1  # the bytewise-last word has one byte


def test_count_tables_shapes():
    (wa, ca), (wb, cb) = C.count_tables()
    want = dict(C.oracle_sum((wa, ca), (wb, cb))[0])
    assert want[b"big"] == (1 << 64) - 1 and want[b"zero"] == 0 and want[b"zf"] == 5
    assert want[b"a_long_word_with_count_zero"] == 0
    assert {c for c in ca if c and c & (c - 1) == 0} >= {1 << i for i in range(64)}
    assert all(bin(want[b"bit%02d" % i]).count("1") == 2 for i in range(64))


def test_oracle_sum_keeps_zero_counts_and_wraps():
    items, tok = C.oracle_sum(([b"a", b"b"], [0, (1 << 64) - 1]), ([b"b", b"c"], [2, 0]))
    assert items == [(b"a", 0), (b"b", 1), (b"c", 0)] and tok == 1


def test_bigger_tables_shapes():
    (wa, _), (wb, _) = C.half_shared(1000)
    assert len(set(wa)) == len(set(wb)) == 1000 and len(set(wa) & set(wb)) == 500
    (la, _), (lb, _) = C.long_tables()
    assert len(set(la) - set(lb)) == 300 and len(set(lb) - set(la)) == 300 and not any(C.is_short(w) for w in la + lb)


def tokens(b):
    return re.split(rb"[ \t\n\x0b\x0c\r]|\xc2\x85|\xe2\x80\x83", b)


@pytest.mark.parametrize("chunk", [0, 256, 300, 1000, 4096, 10 ** 6])
def test_chunk_cut_model(chunk):
    import random
    rng = random.Random(chunk)
    words = [bytes(rng.choice(b"abcdefgh") for _ in range(rng.randint(1, 12))) for _ in range(3000)]
    seps = [b" ", b"\n", b"\t", b"\r\n", b"  ", "\u2003".encode(), "\u0085".encode(), b"\x0b", b"\x0c"]
    text = b"".join(w + rng.choice(seps) for w in words) + b"tail"
    texts = [text, b"", b"x", b"x" * 5000, b"ab " * 2000, b" " * 3000,
             "\u2003".encode().join(words[:400]), "\u0085".encode().join(words[:400])]
    for data in texts:
        ch = C.chunk_cuts(data, chunk)
        assert ch[0][0] == 0 and ch[-1][1] == len(data)
        assert all(a[1] == b[0] for a, b in zip(ch, ch[1:]))  # the chunks concatenate to the input
        assert all(hi > lo for lo, hi in ch) or data == b""
        for lo, hi in ch[1:]:
            assert data[lo - 1] in C.ASCII_WS  # every cut follows an ASCII whitespace byte
            if chunk:
                assert lo >= chunk  # cut k >= k chunk_bytes >= chunk_bytes
        # no token is split: the chunks' tokens are the input's
        parts = [t for lo, hi in ch for t in tokens(data[lo:hi]) if t]
        assert parts == [t for t in tokens(data) if t]
    only_unicode_ws = texts[-2]
    assert len(C.chunk_cuts(only_unicode_ws, chunk)) == 1  # U+2003 is no cut point: one chunk
    assert len(C.chunk_cuts(texts[-1], chunk)) == 1  # nor U+0085
    if chunk == 4096:
        data = (b"word " * 20000)[:65536]
        assert len(C.chunk_cuts(data, 4096)) == 16


def test_docs_mention_the_accumulator():
    for doc, words in (("README.md", ["mox_accumulate", "--chunk"]), ("DESIGN.md", ["mox_accum.hip", "mox_accumulate_file"]),
                       ("INTEGRATION.md", ["mox_accumulate_file", "mox_accum_info"])):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
