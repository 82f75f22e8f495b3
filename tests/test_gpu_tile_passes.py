"""GPU: tile and wave edges of the frame the result operators share
(mox_tiles.h: tile_sums, scan_tiles; the placing round in each kernel): filter, re-key, accumulate,
rank and histogram on tables of an exact row count around the wave, round and
tile sizes.  Tables come from Engine.reduce_pairs and are sorted bytewise, so
row i is words[i]: the last round of a tile (and the last round that holds
rows) carries a word over 64 bytes on the last lane of a wave, a word over 256
bytes on the first lane of the next -- the operators' whole-wave copies, and
long rows of the packers -- and a row with count 0.  Every result is compared
exactly with the operator's model (tests/*_cases.py).  The file runs against
libmox.so and libmox_hc.so (re-key and accumulate have forced-collision
objects)."""
import pytest

import accum_cases
import filter_cases
import hist_cases
import mox
import rank_cases
import rekey_cases

pytestmark = pytest.mark.gpu

ROUND = 256                    # rows of one round of every operator: 4 waves of 64 lanes
TILE = filter_cases.TILE       # the 1,024-row operators: filter, re-key, accumulate
BIG_TILE = rank_cases.TILE     # rank and histogram
assert TILE == rekey_cases.TILE == accum_cases.TILE == 1024 and BIG_TILE == hist_cases.TILE == 4096
NS = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
BIG_NS = (BIG_TILE - 1, BIG_TILE, BIG_TILE + 1, 2 * BIG_TILE + 1)
MIN_COUNT = 10                 # the filter's threshold (see table)
GRID_ENVS = ("MOX_FILTER_GRID", "MOX_REKEY_GRID", "MOX_RANK_GRID", "MOX_HIST_GRID")


@pytest.fixture(scope="module", params=[None, mox.HC_LIB_PATH], ids=["libmox", "libmox_hc"])
def eng(request):
    e = mox.Engine(device=0, lib_path=request.param)
    yield e
    e.close()


def table(n):
    """(words, counts) of n rows, words ascending bytewise.  Every fourth word is
    the one before it plus a trailing "," (re-key with trim=b"," merges the two).
    Counts: rows of the odd 1,024-row tiles are below MIN_COUNT, so with three
    tiles the middle one keeps nothing; of the other tiles' rows every second one
    is kept.  In the last round that holds rows, the last round of the first
    1,024-row tile and that of the first 4,096-row tile: the row of lane 63 of
    the round's first wave is over 64 bytes, the next row (lane 0 of the second
    wave) over 256 bytes, both kept by the filter, and the round's last row has
    count 0 (with fewer rows: as many of the three as fit)."""
    words, counts = [], []
    for i in range(n):
        words.append(words[i - 1] + b"," if i % 4 == 3 else b"r%06d" % i)
        counts.append(1 + i % 5 if (i // TILE) % 2 or i % 2 else 20 + i % 11)
    starts = {(n - 1) // ROUND * ROUND} if n else set()
    starts |= {t - ROUND for t in (TILE, BIG_TILE) if n >= t}
    for r0 in sorted(starts):
        a = min(r0 + 63, n - 1)
        b = a + 1 if a + 1 < n else a - 1
        z = min(r0 + ROUND - 1, n - 1)
        words[a] = b"r%06d" % a + b"x" * 70
        counts[a] = 50
        if b >= r0:
            words[b] = b"r%06d" % b + b"y" * 300
            counts[b] = 51
        if z not in (a, b):
            counts[z] = 0
        for i in (a + 1, b + 1):  # a "," row behind a changed word follows it
            if i < n and i % 4 == 3 and i not in (a, b):
                words[i] = words[i - 1] + b","
    assert words == sorted(words) and len(set(words)) == n
    return words, counts


def load(e, tab):
    """The table as e's resident result with row i = (words[i], counts[i]); the items."""
    e.reduce_pairs(tab[0], tab[1]).close()
    e.sort_result()
    items, _ = accum_cases.fetched(e)
    assert items == list(zip(tab[0], tab[1]))
    return items


def check_small_tile_ops(e, n):
    """Filter, re-key and accumulate twice, each on a fresh copy of table(n)."""
    tab = table(n)
    # filter: with three tiles, one that keeps nothing between two that keep rows
    items = load(e, tab)
    kept, want = filter_cases.expected(items, min_count=MIN_COUNT)
    if n > 2 * TILE:
        tiles = {i // TILE for i, (_, c) in enumerate(items) if c >= MIN_COUNT}
        assert 0 in tiles and 1 not in tiles and 2 in tiles
    long = [w for w in tab[0] if len(w) > 64 and not w.endswith(b",")]  # the whole-wave copies: all of them are kept
    assert [w for w, _ in kept if w in long] == long and (n < 65 or len(long) >= 1 + (n != 257))
    info = e.filter_result(min_count=MIN_COUNT)
    got, tokens = accum_cases.fetched(e)
    assert got == kept and tokens == want["tokens_kept"]
    assert {k: info[k] for k in filter_cases.INFO_KEYS} == want
    # re-key: the "," rows join the rows before them
    items = load(e, tab)
    merged, _, want = rekey_cases.expected(items, trim=b",")
    assert want["words_changed"] == sum(w.endswith(b",") for w in tab[0]) >= (n - 1) // 8 and want["words_dropped"] == 0
    info = e.rekey_result(trim=b",")
    got, tokens = accum_cases.fetched(e)
    assert sorted(got) == sorted(merged) and tokens == want["tokens_out"]
    assert {k: info[k] for k in rekey_cases.INFO_KEYS} == want
    # accumulate twice: the second fold packs the total and the result, n rows each
    e.accumulate_reset()
    for _ in range(2):
        load(e, tab)
        e.accumulate()
    got, tokens = accum_cases.fetched(e)
    info = e.accumulate_info()
    e.accumulate_reset()
    want, wtok = accum_cases.oracle_sum(tab, tab)
    assert (sorted(got), tokens) == (want, wtok)
    assert (info["passes"], info["words"], info["tokens"]) == (2, n, wtok)


def check_big_tile_ops(e, n):
    """Rank descending and the histogram by "bytes", each on a fresh copy of table(n)."""
    tab = table(n)
    items = load(e, tab)
    info = e.rank_result()
    got, _ = accum_cases.fetched(e)
    assert got == rank_cases.expected(items)
    assert {k: info[k] for k in rank_cases.INFO_KEYS} == rank_cases.info_of(items)
    items = load(e, tab)
    want = hist_cases.expected(items, "bytes")
    h = e.histogram("bytes", with_info=True)
    assert list(zip(*(a.tolist() for a in h[:4]))) == want
    assert (h[4], h[5]) == (n, sum(c for _, c in items))
    assert {k: h[6][k] for k in hist_cases.INFO_KEYS} == hist_cases.info_of(want)
    assert accum_cases.fetched(e)[0] == items  # the histogram only reads


@pytest.mark.parametrize("n", NS)
def test_small_tile_operators(eng, n):
    check_small_tile_ops(eng, n)


@pytest.mark.parametrize("n", NS + BIG_NS)
def test_big_tile_operators(eng, n):
    check_big_tile_ops(eng, n)


def test_one_workgroup_walks_the_tiles(eng, monkeypatch):
    """A grid of one: the workgroup takes tile after tile and the shared pieces'
    LDS slots are reused across them."""
    for env in GRID_ENVS:
        monkeypatch.setenv(env, "1")
    check_small_tile_ops(eng, 2 * TILE + 1)
    check_big_tile_ops(eng, 2 * TILE + 1)
    check_big_tile_ops(eng, 2 * BIG_TILE + 1)
