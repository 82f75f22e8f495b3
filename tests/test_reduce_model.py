"""CPU: the hash and geometry model of reduce_cases.py and the cases
test_gpu_reduce_edges.py runs, so that a GPU test there cannot pass while
missing the cut-off it is there for.  The cut-offs are parsed from the kernel
sources; every case is checked to have exactly the units, lists, sub-passes,
buckets and bins it claims; the C oracle counts every corpus to the planned
table (the words are valid UTF-8, free of whitespace and already lowercase).
No GPU code runs here."""
import numpy as np
import pytest

import coracle
import pyoracle
import reduce_cases as R
from reduce_cases import K

ALL = list(R.CORPUS_CASES) + list(R.PAIRS_CASES)


def test_parsed_constants_are_the_ones_the_cases_assume():
    """The cases are laid out for these cut-offs (KK = 5 needs 16 SPLIT_TARGET <
    0.63 (SPLIT_MIN + 1) and SPLIT_MIN + 1208 <= 32 SPLIT_TARGET; the sort keys
    need SMALL_CAP = 512): a change in the sources fails here first."""
    got = {n: getattr(K, n) for n in ("NB_LOG2", "SPLIT_MIN", "SPLIT_TARGET", "SMALL_CAP", "RED_CAP", "RED_BK", "RED_SORTB",
                                      "SUB_BITS_MAX", "SR_TSLOTS", "SR_BIN_BITS", "QF_MAX", "PAY", "DICT_SLOTS",
                                      "DICT_MIN_COVER_INV", "HASH_FIN1", "SAMPLE_PIECE", "SAMPLE_PIECES")}
    assert got == {"NB_LOG2": 10, "SPLIT_MIN": 8192, "SPLIT_TARGET": 320, "SMALL_CAP": 512, "RED_CAP": 2048, "RED_BK": 608,
                   "RED_SORTB": 2048, "SUB_BITS_MAX": 12, "SR_TSLOTS": 1024, "SR_BIN_BITS": 9, "QF_MAX": 4, "PAY": 992,
                   "DICT_SLOTS": 5120, "DICT_MIN_COVER_INV": 20, "HASH_FIN1": 1, "SAMPLE_PIECE": 4096, "SAMPLE_PIECES": 192}
    assert R.RED_BIN_BITS == K.RED_SORTB.bit_length() - 1
    assert R.COLD_CAP % (2 * K.QF_MAX) == 0 and R.GRID * K.QF_MAX <= K.MAX_MAP_GRID  # hc_qf: four slices per region


def test_restated_functions_still_read_as_the_sources_do():
    """The multipliers, shifts and rules restated in reduce_cases.py, found in
    the bodies of the device functions they restate."""
    src = K._k

    def body(sig):
        i = src.index(sig)
        return src[i:src.index("\n}\n", i)]

    assert "0x85EBCA77u" in body("uint32_t hash_fold(") and "21" in body("uint32_t hash_fold(") and ", 6)" in body("uint32_t hash_fold(")
    assert "0x9E3779B1u" in body("uint32_t hash_fin(") and "a >> 16" in body("uint32_t hash_fin(")
    assert "max(collide32(a, MOX_H32_BITS), 1u)" in body("uint32_t hash32(")
    hb = body("uint32_t hash32b(")
    for c in ("0x2127599Bu", "0x165667B1u", "0xD3A2646Du", "0x2C1B3C6Du", "a >> 12", "0x297A2D39u", "a >> 15"):
        assert c in hb
    assert "(h & 0xFFFFu) * (uint32_t)RED_BK) >> 16" in src
    assert "(h << shift) >> (32 - 11)" in src
    assert "(h * 0x9E3779B1u) >> (32 - 10)" in src
    assert "d[j] == 0 && c[j] > SMALL_CAP && c[j] <= 2 * SMALL_CAP" in src and "c[j] + d[j] > SMALL_CAP" in src
    assert "nc + nw <= SPLIT_MIN" in src and "est > (float)SPLIT_TARGET * (float)(1u << kk)" in src and "r >= 0.5f" in src
    assert "(h << shift) | (hb >> (32 - shift))" in src
    assert R.FIN_MUL * R.FIN_INV % (1 << 32) == 1
    a = np.arange(0, 1 << 32, 104729, dtype=np.uint64)
    assert np.array_equal(R.hash_unfin(R.hash_fin(a)), a.astype(np.uint32))


def test_hash_model_known_values():
    """Hand-computed: the key of b"a" is k0 = 0x61, the rest 0."""
    k0 = 0x61
    t = k0 * 0x9E3779B1 % (1 << 32)
    assert int(R.hash32(k0, 0, 0, 0)[0]) == t ^ (t >> 16)
    assert R.pack([b"abcdefghi"]).tolist() == [[0x64636261, 0x68676665, 0x69, 0]]
    fold = (1 ^ (2 * 0x85EBCA77) ^ (3 << 21) ^ (4 << 6)) % (1 << 32)
    assert int(R.hash_fold(1, 2, 3, 4)[0]) == fold
    assert int(R.hash_fold(0, 0, 0x80000000, 0x80000000)[0]) == (1 << 20) ^ (1 << 5)  # the rotations wrap
    assert int(R.hash32(0, 0, 0, 0)[0]) == 1 and int(R.hash_raw(0, 0, 0, 0)[0]) == 0
    assert int(R.red_bucket(0xFFFF)) == K.RED_BK - 1 and int(R.red_bucket(0x12340000)) == 0
    assert int(R.hbits(0xFFC00000, 0, 10)) == 1023 and int(R.hbits(0x00200000, 10, 1)) == 1 and int(R.hbits(5, 32, 3)) == 0


def check_words(words, h32, mask, nonascii, raw=False):
    assert len(set(words)) == len(words)
    x = R.Hashed(words)
    hash_ = x.raw if raw else x.h
    assert ((hash_ ^ np.uint32(h32)) & np.uint32(mask)).max() == 0
    for w in words:
        assert (6 if nonascii else 5) <= len(w) <= 8
        assert all(b in R.ALPHA for b in w[:4]) and b"\0" not in w
        tail = w[4:]
        if nonascii:
            assert tuple(tail[:2]) in {tuple(p) for p in R.PAIRS2.tolist()}
            tail = tail[2:]
        assert all(b in R.ALPHA for b in tail)
        assert coracle.lowercase(w) == w and w.decode("utf-8").lower().encode() == w
    assert [t.encode() for t in pyoracle.split_whitespace(b" ".join(words).decode())] == words


@pytest.mark.parametrize("h32,mask,n,nonascii,raw", [
    (0xDEADBEEF, R.M32, 300, False, False),
    (0x00000001, R.M32, 50, False, False),      # the clamp: raw hashes 0 and 1
    (0x00000000, R.M32, 50, False, True),
    (0x00000001, R.M32, 50, False, True),
    (0x2A300000, R.part_mask(), 2049, False, False),
    (R.unit_hash(0x155, 5, 17), R.unit_mask(5), 1025, False, False),
    (0x0000FFFF, 0x0000FFFF, 40, False, False),
    (R.unit_hash(0x0C7, 5, 19), R.unit_mask(5), 513, True, False),
    (0x12345678, 0, 5000, False, False),
])
def test_words_for_round_trips(h32, mask, n, nonascii, raw):
    words = R.words_for(h32, n, mask=mask, nonascii=nonascii, raw=raw, seed=3)
    assert len(words) == n
    check_words(words, h32, mask, nonascii, raw)
    assert words == R.words_for(h32, n, mask=mask, nonascii=nonascii, raw=raw, seed=3)  # seeded
    if raw and mask == R.M32:
        assert set(R.Hashed(words).h.tolist()) == {max(h32, 1)}


def test_words_for_full_hash_non_ascii_and_failure():
    h, words = R.hash_with_words(0x6D880000, 16, 100, seed=1, nonascii=True)
    check_words(words, h, R.M32, True)
    with pytest.raises(R.CannotBuild):
        R.words_for(0x6D880F0F, 1, nonascii=True, tries=2)  # no lead byte gives this hash a printable first byte


@pytest.mark.parametrize("name", ALL)
def test_case_counts_to_its_plan_under_the_oracle(name):
    """The corpus of the case, counted by the C oracle, is the planned table:
    every word is valid UTF-8 without whitespace and unchanged by lowering."""
    c = R.case(name)
    want = sorted(c.expected().items())
    if c.pairs is not None:
        assert all(len(w) <= 16 and b"\0" not in w for w, _ in c.pairs)
        return
    text = c.text()
    assert K.SAMPLE_PIECES * (K.SAMPLE_PIECE + 16) <= len(text) < 1 << 20  # the dictionary sample's pieces do not overlap
    got, tokens = coracle.count(text)
    assert got == want and tokens == sum(cnt for _, cnt, _ in c.items)
    assert all((max(w) >= 0x80) == bool(f) for w, _, f in c.items)  # weighted here = through the Unicode lane
    assert dict(pyoracle.count_words(text[:20000])) == {k.decode(): v for k, v in coracle.count(text[:20000])[0]}


@pytest.mark.parametrize("name", ALL)
def test_case_geometry_is_the_claimed_one(name):
    c = R.case(name)
    g, cl = c.geometry, c.claims
    s = g.summary()
    if "summary" in cl:
        assert {k: s[k] for k in cl["summary"]} == cl["summary"]
    if "summary_dict" in cl:
        sd = c.dict_geometry.summary()
        assert {k: sd[k] for k in cl["summary_dict"]} == cl["summary_dict"]
        assert sd["cold_records"] == s["cold_records"] - sum(n for w, n, _ in c.items if w in c.hot)
        assert all(n >= 2 * 256 for w, n, _ in c.items if w in c.hot)       # sampled counts stay over 255 ...
        assert all(n < 64 for w, n, _ in c.items if w not in c.hot)         # ... and no other word's gets near
    for sub, n in cl.get("unit_records", {}).items():
        u = g.unit(cl["part"], sub)
        assert u.records == n and u.kk == R.KK, (sub, u.records)
    for sub, where in cl.get("unit_lists", {}).items():
        assert g.unit(cl["part"], sub).list == where, sub
    for p, n in cl.get("whole", {}).items():
        assert g.kk[p] == 0 and g.records[p] == n
    for p, n in cl.get("split_parts", {}).items():
        assert g.kk[p] == R.KK and g.records[p] == n
    # no split partition sits near a kk boundary: kk is the same for every
    # sampled distinct fraction from 0.63 up, and the true fraction is above 0.8
    exp = c.expected()
    x = R.Hashed(list(exp))
    part = R.bucket_of(x.h).astype(np.int64)
    for b in np.nonzero(np.array(g.kk))[0]:
        tot = int(g.records[b])
        assert K.SPLIT_MIN < tot <= 32 * K.SPLIT_TARGET
        assert R.kk_for(tot, 0.63) == R.kk_for(tot, 1.0) == R.KK
        assert int((part == b).sum()) >= 0.8 * tot
    # no two words share (h32, hash32b): such a unit would move to k_reduce's list
    assert len(set(zip(x.h.tolist(), x.hb.tolist()))) == len(x.words)
    if c.pairs is None and c.default_engine != "exact":
        # no region slice overflows at the reserved capacity (a spill would turn cold records into weighted ones)
        assert c.region_fill() <= R.COLD_CAP // K.QF_MAX - 4
    if c.default_engine in ("same", "hot") and c.pairs is None:
        assert c.repeat_fraction() <= 0.8 / K.DICT_MIN_COVER_INV  # no dictionary forms


@pytest.mark.parametrize("name", ALL)
def test_model_order_is_a_strict_total_order(name):
    words = list(R.case(name).expected())
    order = R.model_order(words)
    keys = [R.order_key(w) for w in order[:2000]] + [R.order_key(w) for w in order[-500:]]
    x = R.Hashed(order)
    allk = list(zip(x.h.tolist(), x.hb.tolist(), x.w0.tolist(), x.w1.tolist()))
    assert sorted(set(order)) == sorted(words)
    assert all(a < b for a, b in zip(allk, allk[1:]))  # strictly ascending: irreflexive, total, transitive
    assert keys == allk[:2000] + allk[-500:]


def test_unit_sizes_details():
    c = R.case("unit_sizes")
    g, P = c.geometry, c.claims["part"]
    assert sorted(u.records for u in g.units.values() if u.part == P and u.cold and not u.weighted)[-1] == 1025
    assert {0, 1, 64, 65, 511, 512, 513, 1023, 1024, 1025} <= {g.unit(P, s).records for s in range(32)}
    assert 9100 <= g.records[P] <= 9700
    x = R.Hashed([w for w, _, _ in c.items])
    sub = np.where(R.bucket_of(x.h) == P, R.hbits(x.h, K.NB_LOG2, R.KK).astype(np.int64), -1).tolist()
    copies = {s: sorted((it[1] for it, u in zip(c.items, sub) if u == s), reverse=True)[:2] for s in (1, 2, 16, 17)}
    assert copies == {1: [512], 2: [9, 1], 16: [1024], 17: [17, 1]}
    # the four slices of the partition's regions carry about a quarter each
    per = [sum(g.unit(P, s).records for s in range(8 * q, 8 * q + 8)) for q in range(4)]
    assert max(per) - min(per) < 64


def test_sort_key_ties_details():
    c = R.case("sort_key_ties")
    for sub, groups in c.claims["tie_groups"].items():
        per = c.claims["per"][sub]
        assert [len(ws) for ws, _ in groups] == [2, 5, 2, 5]
        for ws, same in groups:
            x = R.Hashed(ws)
            assert len(set(x.h.tolist())) == 1 and len(set(x.hb.tolist())) == len(ws)
            assert int(R.bucket_of(x.h)[0]) == c.claims["part"] and int(R.hbits(x.h, 10, 5)[0]) == sub
            keys = set(R.sort_key_bits(x.h, x.hb, R.KK, per).tolist())
            assert len(keys) == (1 if same else len(ws))


def test_bucket_clusters_details():
    c = R.case("bucket_clusters")
    cl, parts = c.claims["clusters"], c.claims["parts"]
    g = c.geometry
    distinct = np.bincount(R.bucket_of(R.Hashed(list(c.expected())).h).astype(np.int64), minlength=K.NB)
    for name, ws in cl.items():
        x = R.Hashed(ws)
        assert set(R.bucket_of(x.h).tolist()) == {parts[name]}
        assert 200 < g.records[parts[name]] and distinct[parts[name]] < K.RED_CAP
    for name, n in (("tag9", 9), ("tag12", 12), ("tag40", 40)):
        x = R.Hashed(cl[name])
        assert len(x.words) == n > 8 and len(set(x.h.tolist())) == 1  # more than its two buckets' eight slots
    x = R.Hashed(cl["low16"])
    assert len(x.words) == 40 and len(set(R.red_bucket(x.h).tolist())) == 1 and len(set(x.h.tolist())) > 20
    x = R.Hashed(cl["wrap"])
    assert len(x.words) == 20 and set(R.red_bucket(x.h).tolist()) == {K.RED_BK - 1} and len(set(x.h.tolist())) == 1
    assert -(-20 // 4) > 2  # buckets RED_BK - 1, the spare one, then 0, 1, 2
    x = R.Hashed(cl["bin"])
    assert len(x.words) == 100 and len(set(R.red_bin(x.h, K.NB_LOG2).tolist())) == 1 and len(set(x.h.tolist())) > 90


def test_small_table_clusters_details():
    c = R.case("small_table_clusters")
    cl = c.claims
    x = R.Hashed(cl["chain"])
    assert len(x.words) == 100 and len(set(x.h.tolist())) == 1
    x = R.Hashed(cl["wrap"])
    assert set(R.sr_slot(x.h).tolist()) == {K.SR_TSLOTS - 1} and len(set(x.h.tolist())) == 3 and len(x.words) == 12
    assert dict((w, n) for w, n, _ in c.items)[cl["hot"]] == 300
    assert all(max(w) >= 0x80 for w in cl["chain"] + cl["wrap"] + [cl["hot"]])


def test_hash_zero_and_dictionary_details():
    c = R.case("hash_zero")
    assert R.Hashed(c.claims["raw0"]).raw.tolist() == [0, 0] and R.Hashed(c.claims["raw1"]).raw.tolist() == [1, 1, 1]
    assert set(R.Hashed(c.claims["raw0"] + c.claims["raw1"]).h.tolist()) == {1}
    exp = c.expected()
    assert sorted(exp[w] for w in c.claims["raw0"] + c.claims["raw1"])[:3] == [1, 1, 1]
    assert sum(exp[w] > 1000 for w in c.claims["raw0"]) == 1 and sum(exp[w] > 1000 for w in c.claims["raw1"]) == 1
    assert R.dict_placed(c.hot) == len(c.hot) - 1  # hashes 0 and 1 share both their slots (slot 0)
    d = R.case("dictionary_same_hash")
    x = R.Hashed(d.claims["same"])
    assert len(x.words) == 7 and set(x.h.tolist()) == {d.claims["h32"]}
    assert sum(d.expected()[w] > 1000 for w in d.claims["same"]) == 4
    assert R.dict_placed(d.hot) == len(d.hot) - 2  # two slots for four words


def test_pairs_case_details():
    c = R.case("pairs_split_min")
    exp = c.expected()
    assert len(c.pairs) == 2 * K.SPLIT_MIN + 1 and len(exp) < len(c.pairs)  # duplicate words sum
    vals = [n for _, n in c.pairs]
    assert (1 << 32) - 1 in vals and (1 << 53) + 1 in vals and vals.count(1 << 62) == 2
    assert 1 << 63 in exp.values() and max(exp.values()) < 1 << 64
    sizes = sorted(c.claims["unit_records"].values())
    assert sizes.count(K.SMALL_CAP) == 7 and sizes.count(K.SMALL_CAP + 1) == 6 and sizes[-1] == K.SMALL_CAP + 1


def test_moving_a_unit_off_its_edge_is_noticed():
    """The 513-record unit of unit_sizes made 512 records: the lists the case
    claims no longer hold (the check the GPU test makes against the device)."""
    c = R.case("unit_sizes")
    P = c.claims["part"]
    x = R.Hashed([w for w, _, _ in c.items])
    in9 = (R.bucket_of(x.h) == P) & (R.hbits(x.h, 10, 5) == 9)
    drop = int(np.nonzero(in9)[0][0])
    moved = R.Geometry([it for i, it in enumerate(c.items) if i != drop])
    assert moved.unit(P, 9).records == 512 and moved.unit(P, 9).list == R.SORT1
    assert moved.summary()["sort2"] == c.claims["summary"]["sort2"] - 1
    # and one record more in the whole partition of split_min_edge splits it
    e = R.case("split_min_edge")
    (A, n), = e.claims["whole"].items()
    extra = R.words_for(A << 22, 1, mask=R.part_mask(), seed=99)[0]
    assert extra not in e.expected()
    assert R.Geometry(e.items + [(extra, 1, False)]).summary()["split"] == 2
