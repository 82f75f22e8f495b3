"""GPU: the carry of every one-workgroup scan over the device-resident table
(mox_dev.h: scan_one_wg behind k_tk_scan, k_tx_scan and k_ac_scan; mox_tiles.h:
the wider scan_tiles behind k_fl_scan and k_rekey_scan).  One corpus, rank_cases.BIG_CORPUS bytes of HICARD text: about
6.04 M distinct words, so the table is past one step of the top-k scan (1,024
tiles of 4,096 rows) and of the filter and re-key scans (4,096 tiles of 1,024 rows), and
nearly six steps of the text and accumulate scans (1,024 tiles of 1,024 rows);
it holds words over 16 bytes, so the accumulate packer's long-row arrays are
scanned with a carry too.  Every check is exact and runs over numpy arrays;
the expectation comes from a fetch of the same run (the engine order of words
longer than 16 bytes can differ from run to run)."""
import numpy as np
import pytest

import accum_cases
import filter_cases
import mox
import rank_cases
import rekey_cases
import text_cases
import top_cases
from mox import corpus

pytestmark = pytest.mark.gpu

FILTER_SCAN_STEP = 4096  # FL_SCAN_STEP: tiles per step of k_fl_scan
REKEY_SCAN_STEP = 4096   # RQ_SCAN_STEP: tiles per step of k_rekey_scan
SCAN_STEP = 1024         # tiles per step of scan_one_wg in k_tk_scan, k_tx_scan, k_ac_scan


@pytest.fixture(scope="module")
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return corpus.fill(corpus.HICARD, 17, 0, rank_cases.BIG_CORPUS).tobytes()


def arrays_of(t):
    """(counts, offs, bytes as a uint8 array) of a Table, which is closed."""
    counts, offs, text = t.arrays()
    t.close()
    return counts, offs, np.frombuffer(text, np.uint8)


def run(eng, data):
    """A fresh run; its table as arrays, the result stays on the device."""
    t = eng.count(data)
    tokens = t.tokens
    return arrays_of(t) + (tokens,)


def test_text(eng, data, tmp_path):
    counts, offs, text, _ = run(eng, data)
    assert len(counts) > SCAN_STEP * text_cases.TILE
    t = eng.fetch()
    path = tmp_path / "final_result.txt"
    t.write_final_result(str(path))
    t.close()
    assert eng.result_text() == path.read_bytes()


def test_top_words(eng, data):
    counts, offs, text, tokens = run(eng, data)
    n = len(counts)
    assert n > SCAN_STEP * top_cases.TILE
    k = top_cases.TOP_MAX
    order = np.argsort(-counts.astype(np.int64), kind="stable")[:k]
    # the threshold count's ties lie in tiles past the first step of the scan
    assert (np.flatnonzero(counts == counts[order[-1]]) // top_cases.TILE).max() >= SCAN_STEP
    t = eng.top_words(k)
    assert (t.n, t.tokens) == (k, tokens)
    got_c, got_o, got_b = arrays_of(t)
    lens = (offs[1:] - offs[:-1])[order]
    assert np.array_equal(got_c, counts[order])
    assert np.array_equal(got_o, np.concatenate(([0], np.cumsum(lens))).astype(np.uint64))
    assert got_b.tobytes() == b"".join(text[int(offs[i]):int(offs[i + 1])].tobytes() for i in order)


@pytest.mark.parametrize("pred", ["min_count", "prefix"])
def test_filter(eng, data, pred):
    counts, offs, text, _ = run(eng, data)
    n = len(counts)
    assert n > FILTER_SCAN_STEP * filter_cases.TILE
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    if pred == "min_count":
        mask = counts >= 2
        info = eng.filter_result(min_count=2)
    else:
        mask = (lens > 0) & (text[np.minimum(offs[:-1], len(text) - 1).astype(np.int64)] == ord("a"))
        info = eng.filter_result(prefix=b"a")
    kept = int(mask.sum())
    assert 0 < kept < n and (np.flatnonzero(mask) // filter_cases.TILE).max() >= FILTER_SCAN_STEP  # kept rows behind the carry
    assert (info["words_in"], info["words_kept"], info["tokens_kept"], info["bytes_kept"]) == \
        (n, kept, int(counts[mask].sum()), int(lens[mask].sum()))
    got_c, got_o, got_b = arrays_of(eng.fetch())
    assert np.array_equal(got_c, counts[mask])
    assert np.array_equal(got_o, np.concatenate(([0], np.cumsum(lens[mask]))).astype(np.uint64))
    assert np.array_equal(got_b, text[np.repeat(mask, lens)])


def test_rekey(eng, data):
    """max_chars=3: every word becomes its first three characters and the rows
    that became equal are summed; rows behind the scan's first step change."""
    counts, offs, text, tokens = run(eng, data)
    n = len(counts)
    assert n > REKEY_SCAN_STEP * rekey_cases.TILE
    assert 0 < int(text.min()) and int(text.max()) < 0x80  # characters are bytes, and none is NUL: a key below orders as its bytes do
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    assert int(lens.min()) >= 1
    assert (np.flatnonzero(lens > 3) // rekey_cases.TILE).max() >= REKEY_SCAN_STEP  # changed rows behind the carry
    # a word's first min(len, 3) bytes, the first one highest: integer order is bytewise order
    at = offs[:-1].astype(np.int64)
    key = np.zeros(n, dtype=np.int64)
    for j in range(3):
        key |= np.where(lens > j, text[np.minimum(at + j, len(text) - 1)].astype(np.int64), 0) << (16 - 8 * j)
    order = np.argsort(key, kind="stable")
    keys, starts = np.unique(key[order], return_index=True)
    want_c = np.add.reduceat(counts[order], starts)
    want_l = 1 + ((keys >> 8) & 255 != 0) + (keys & 255 != 0)
    want_b = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)
    want_b = want_b[np.arange(3)[None, :] < want_l[:, None]]
    info = eng.rekey_result(max_chars=3)
    assert (info["words_in"], info["words_out"], info["tokens_out"], info["words_dropped"]) == (n, len(keys), tokens, 0)
    assert info["words_changed"] == int((lens > 3).sum())
    eng.sort_result()
    got_c, got_o, got_b = arrays_of(eng.fetch())
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_o, np.concatenate(([0], np.cumsum(want_l))).astype(np.uint64))
    assert np.array_equal(got_b, want_b)


def test_accumulate_twice(eng, data):
    eng.accumulate_reset()
    eng.count(data).close()
    eng.sort_result()
    counts, offs, text = arrays_of(eng.fetch())
    n = len(counts)
    assert n > SCAN_STEP * accum_cases.TILE  # both sources of the second fold
    assert int((offs[1:] - offs[:-1]).max()) > 16  # long rows: their two tile arrays are scanned with a carry too
    eng.accumulate_reset()
    for _ in range(2):
        eng.count(data).close()
        eng.accumulate()
    eng.sort_result()
    info = eng.accumulate_info()
    got_c, got_o, got_b = arrays_of(eng.fetch())
    eng.accumulate_reset()
    assert (info["passes"], info["words"]) == (2, n)
    assert np.array_equal(got_o, offs) and np.array_equal(got_b, text)
    assert np.array_equal(got_c, 2 * counts)
