"""The two helpers the Python binding's calls over the result share: an info
struct as a dict, and the validation of a packed word list.  No library is
loaded."""
import numpy as np
import pytest

import mox


def test_info_dict():
    f = mox.FilterInfo()
    f.words_in, f.words_kept, f.tokens_in, f.tokens_kept, f.bytes_kept, f.list_found, f.device_bytes, f.ms = 9, 8, 7, 6, 5, 4, 3, 1.5
    f.reserved[0] = 99
    d = mox._info_dict(f)
    assert d == {"words_in": 9, "words_kept": 8, "tokens_in": 7, "tokens_kept": 6, "bytes_kept": 5, "list_found": 4,
                 "device_bytes": 3, "ms": 1.5}
    assert type(d["ms"]) is float and all(type(v) is int for k, v in d.items() if k != "ms")
    h = mox.HistInfo()
    h.words, h.tokens, h.bins, h.max_key, h.digit_passes, h.device_bytes, h.ms = 1 << 40, (1 << 64) - 1, 3, 1 << 63, 8, 2, 0.25
    d = mox._info_dict(h)
    assert d == {"words": 1 << 40, "tokens": (1 << 64) - 1, "bins": 3, "max_key": 1 << 63, "digit_passes": 8, "device_bytes": 2,
                 "ms": 0.25}
    assert type(d["ms"]) is float and "reserved" not in d
    a = mox.AccumInfo()
    a.passes, a.words, a.tokens, a.device_bytes = 2, 3, 4, 5
    assert mox._info_dict(a) == {"passes": 2, "words": 3, "tokens": 4, "device_bytes": 5}


def test_packed():
    buf, offs, n = mox._packed(b"abcde", [0, 2, 5], "words")
    assert (buf.dtype, offs.dtype, n) == (np.uint8, np.uint64, 2) and buf.tobytes() == b"abcde" and offs.tolist() == [0, 2, 5]
    buf, offs, n = mox._packed(np.frombuffer(b"xy", np.uint8), np.array([0, 2], np.uint64), "keys")
    assert n == 1 and buf.tobytes() == b"xy"
    buf, offs, n = mox._packed(b"", [0], "words")  # an empty list
    assert n == 0 and buf.size == 0
    with pytest.raises(TypeError):
        mox._packed(None, [0], "words")  # (filter_result_packed alone takes None, and passes b"")
    with pytest.raises(ValueError, match=r"^offs needs n \+ 1 entries$"):
        mox._packed(b"ab", [], "words")  # n < 0
    with pytest.raises(ValueError, match=r"^offsets run past the words' bytes$"):
        mox._packed(b"ab", [0, 3], "words")
    with pytest.raises(ValueError, match=r"^offsets run past the keys' bytes$"):
        mox._packed(b"", [0, 1], "keys")
