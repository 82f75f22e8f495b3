"""Host side of the multi-GPU path: byte-range sharding with
word-boundary halos, a gloo all-to-all for the host-staged exchange and
gather transport (mox_exchange_host / mox_gather_host), and a checker-side
merge of per-rank tables.  The gather itself is device side (mox_gather).

The reference runs one process (main.rs:16-22); sharding is this engine's
addition.  Every token belongs to the rank whose byte range holds its first
byte; a rank's buffer carries 64 bytes of left context and HALO bytes of
look-ahead so it can finish its last token (the engine reports MOX_EHALO,
mox.HaloError, if a token runs past the look-ahead: it ends at or after the
buffer end, or the whitespace character after it is cut there).  A character
whose first byte is owned and that the end of a non-final buffer cuts is
MOX_EHALO too, even inside a token of the rank before.
"""
import heapq

LEFT_CONTEXT = 64
HALO = 1 << 16


def shard_range(total, world, rank, per_rank=None, halo=HALO):
    """(lo, hi, own_begin, own_end, at_end) of rank's shard of a corpus of
    ``total`` bytes: buffer = corpus[lo:hi], owned bytes = [own_begin, own_end)
    relative to lo.  ``per_rank`` fixes the shard size (weak scaling); default
    splits ``total`` evenly."""
    if per_rank is None:
        # >= 4 so that every non-first owned range has the engine's minimum
        # left context (mox_run_range: own_begin is 0 or >= 4)
        per_rank = max(4, (total + world - 1) // world)
    ob = min(total, rank * per_rank)
    oe = min(total, ob + per_rank) if rank < world - 1 else total
    if ob == oe:  # nothing owned: an empty buffer at the corpus end
        return total, total, 0, 0, True
    lo = max(0, ob - LEFT_CONTEXT)
    hi = min(total, oe + halo)
    return lo, hi, ob - lo, oe - lo, hi == total


def gloo_alltoallv(group=None):
    """An ``alltoallv(send, send_sizes, recv_sizes)`` for Engine.exchange_host over
    torch.distributed (CPU tensors; gloo)."""
    import numpy as np
    import torch
    import torch.distributed as dist

    def a2a(send, send_sizes, recv_sizes):
        inp = torch.from_numpy(np.frombuffer(send, dtype=np.uint8).copy()) if sum(send_sizes) else torch.empty(0, dtype=torch.uint8)
        out = torch.empty(sum(recv_sizes), dtype=torch.uint8)
        dist.all_to_all_single(out, inp, list(recv_sizes), list(send_sizes), group=group)
        return out.numpy().tobytes()

    return a2a


def merge_tables(parts):
    """k-way merge of per-rank (word, count) lists, each sorted bytewise, into one
    bytewise-sorted list.  Ranks own disjoint words after the exchange; a word
    seen on two ranks is an error (it would mean a wrong owner mapping)."""
    out = []
    for w, c in heapq.merge(*parts, key=lambda kv: kv[0]):
        if out and out[-1][0] == w:
            raise ValueError("word %r owned by two ranks" % (w,))
        out.append((w, c))
    return out


def merge_top(parts, k):
    """Global top-k from per-rank top-k lists: ``parts[r]`` is rank r's
    ``Engine.top_words(k)`` as a list of (word, count).  Ranks own disjoint
    words after the exchange, so the global top-k is the top-k of the union,
    by (count descending, rank ascending, position in the rank's list
    ascending) -- the tie order mox_gather in rank order followed by
    mox_top_words gives, without gathering the table.  A word in two parts is
    an error, as in merge_tables."""
    seen, rows = set(), []
    for r, part in enumerate(parts):
        for pos, (w, c) in enumerate(part):
            if w in seen:
                raise ValueError("word %r owned by two ranks" % (w,))
            seen.add(w)
            rows.append((-c, r, pos, w))
    rows.sort(key=lambda t: t[:3])
    return [(w, -c) for c, _, _, w in rows[:max(k, 0)]]


def sum_lookups(parts, found=None):
    """Global counts from per-rank lookups: ``parts[r]`` is rank r's
    ``Engine.lookup(words)`` of the same words after the exchange.  Ranks own
    disjoint words then, so the element-wise sum is the count a gather followed by
    one lookup gives, without gathering -- the lookup counterpart of merge_top.
    Returns a numpy uint64 array; ValueError when the lengths differ.
    ``found[r]`` (optional) is rank r's mask ``index != LOOKUP_NONE``: a word two
    ranks both found is an error, as in merge_tables."""
    import numpy as np

    arrs = [np.asarray(p, dtype=np.uint64).reshape(-1) for p in parts]
    if not arrs:
        return np.zeros(0, dtype=np.uint64)
    if any(a.size != arrs[0].size for a in arrs):
        raise ValueError("per-rank lookups differ in length: %r" % ([a.size for a in arrs],))
    if found is not None:
        masks = [np.asarray(m, dtype=bool).reshape(-1) for m in found]
        if len(masks) != len(arrs) or any(m.size != arrs[0].size for m in masks):
            raise ValueError("found masks do not match the lookups")
        owners = np.sum(masks, axis=0, dtype=np.int64) if masks else np.zeros(arrs[0].size, np.int64)
        if (owners > 1).any():
            raise ValueError("query %d found on two ranks" % int(np.argmax(owners > 1)))
    total = np.zeros(arrs[0].size, dtype=np.uint64)
    for a in arrs:
        total += a
    return total


def sum_finds(per_rank):
    """Global (rows, sums) from per-rank finds: ``per_rank[r]`` is rank r's
    ``Engine.find(keys, mode)`` -- (first, last) or (first, last, sums) -- of the
    same keys after a ranged exchange.  Each rank then owns a byte range of the
    words, so the ranks' ``last - first`` and ``sums`` add up (sums wrapping, as on
    the device) to what a gather followed by one find gives, without gathering.
    Returns two numpy uint64 arrays; sums is None when a rank's tuple has none.
    ValueError when the lengths differ."""
    import numpy as np

    parts = [tuple(np.asarray(a, dtype=np.uint64).reshape(-1) for a in p[:3]) for p in per_rank]
    if not parts:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    n = parts[0][0].size
    if any(a.size != n for p in parts for a in p):
        raise ValueError("per-rank finds differ in length")
    rows = np.zeros(n, dtype=np.uint64)
    sums = np.zeros(n, dtype=np.uint64) if all(len(p) == 3 for p in parts) else None
    for p in parts:
        rows += p[1] - p[0]
        if sums is not None:
            sums += p[2]
    return rows, sums


def sum_histograms(parts):
    """Global bins from per-rank histograms: ``parts[r]`` is rank r's
    ``Engine.histogram(key)`` -- (keys, bin_words, bin_tokens, ...) -- of the same
    key after an exchange.  The ranks then own disjoint words, so bins merge by
    key and their words and tokens add up (wrapping as u64, as on the device) to
    what a gather followed by one histogram gives, without gathering.  Returns
    (keys, bin_words, bin_tokens, words, tokens): keys ascending; first_row is per
    rank and is dropped.  ValueError when a part's arrays differ in length."""
    import numpy as np

    arrs = [tuple(np.asarray(a, dtype=np.uint64).reshape(-1) for a in p[:3]) for p in parts]
    if any(len(p) < 3 or p[0].size != p[1].size or p[0].size != p[2].size for p in arrs):
        raise ValueError("a histogram needs keys, bin_words and bin_tokens of one length")
    if not arrs:
        z = np.zeros(0, dtype=np.uint64)
        return z, z.copy(), z.copy(), 0, 0
    keys, inv = np.unique(np.concatenate([p[0] for p in arrs]), return_inverse=True)
    words = np.zeros(keys.size, dtype=np.uint64)
    tokens = np.zeros(keys.size, dtype=np.uint64)
    np.add.at(words, inv, np.concatenate([p[1] for p in arrs]))  # (unsigned adds wrap)
    np.add.at(tokens, inv, np.concatenate([p[2] for p in arrs]))
    return keys, words, tokens, int(words.sum(dtype=np.uint64)), int(tokens.sum(dtype=np.uint64))


def sum_joins(infos):
    """The global join info from per-rank joins: ``infos[r]`` is rank r's
    ``Engine.join_total(...)`` after a hash-owner exchange (no MOX_F_SORT_BYTES),
    where every rank accumulates its exchanged results: a word's owner is the
    same rank in every window, so the ranks' words, tokens and overlap sums add up
    (wrapping, as on the device) to what a gather followed by one join gives.
    ``device_bytes`` and ``ms`` are not additive: the largest is reported.  With
    ranged owners a local join is wrong: gather first."""
    infos = list(infos)
    out = {}
    for info in infos:
        for k, v in info.items():
            if k in ("device_bytes", "ms"):
                out[k] = max(out.get(k, v), v)
            else:
                out[k] = (out.get(k, 0) + v) & ((1 << 64) - 1)
    return out


class ThreadAlltoall:
    """In-process all-to-all between ``world`` threads (one engine per thread),
    for exercising the exchange with several ranks on one GPU without a process
    group.  ``fn(rank)`` is the alltoallv callback of that rank's thread."""

    def __init__(self, world):
        import threading

        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world

    def fn(self, rank):
        def a2a(send, send_sizes, recv_sizes):
            data = bytes(send)
            offs = [0]
            for s in send_sizes:
                offs.append(offs[-1] + s)
            self.slots[rank] = [data[offs[d]:offs[d + 1]] for d in range(self.world)]
            self.barrier.wait()
            out = b"".join(self.slots[s][rank] for s in range(self.world))
            self.barrier.wait()  # every rank has read before the slots are reused
            if len(out) != sum(recv_sizes):
                raise ValueError("size mismatch in ThreadAlltoall")
            return out

        return a2a
