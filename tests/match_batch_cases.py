"""Shared cases of tests/test_match_batch.py (emulator) and tests/test_gpu_match_batch.py (MI355X): gsh_match_orb_batch
against the oracle's gs_match_orb, pair by pair and bit for bit.

`g` is a bound library, `mem` a parity_cases.Mem ("host": the emulator takes host memory for device memory; "device": torch
CUDA tensors), `oracles` the CPU oracles that must all give the expected records (the C restatement, and the compiled
reference wherever oracle/_ref was built).

Every run (`run`): descriptors come from parity_cases.random_descriptors (partners at distance 0 / 3 / 40, some of them
twice in the train set), pair by pair under a different XOR mask and train order, so that no two pairs of a batch are the
same; the record slots beyond a set's device-side count hold exact partners of the other set, so a kernel that reads one
finds other matches; matches and counts are pre-filled with 0x5a inside larger guarded buffers, and the records at and
beyond counts[p] must come back as they were; k1, k2 and the counts are compared with their copies afterwards.

The kernel's split of a pair's train range (k_match.h: kMatchTile, kMatchSlices) is restated in `plan`, so that every case
can say how many waves of a block work and how many tiles the longest slice has."""
import numpy as np

from geom_batch_cases import FILL, Guarded, sync
from grayskull_amd import KEYPOINT_DTYPE
from parity_cases import random_descriptors

T, S = 64, 16  # kMatchTile: train descriptors per staged tile; kMatchSlices: waves of a block = slices of the train range
TRAIN_SIZES = (0, 1, T - 1, T, T + 1, 2 * T + 1, S * T + 1)
QUERY_SIZES = (0, 1, 63, 64, 65, 129, 2049)  # 2049: two compaction chunks (kChunkWords * 64 = 2048)


def plan(nt):
    """(descriptors per slice, waves with a non-empty slice, tiles of a full slice) for nt train descriptors"""
    if nt == 0:
        return 0, 0, 0
    length = (nt - 1) // S + 1
    return length, (nt + length - 1) // length, (length + T - 1) // T


def raw(k):
    return k.view(np.uint32).reshape(len(k), 12)


def records(r):
    """(n, 12) uint32 -> n keypoint records for the oracle (a view: the address stays valid for n == 0)"""
    return np.ascontiguousarray(r).view(KEYPOINT_DTYPE).reshape(-1)


def pair(nq, nt, salt=0):
    """(queries (nq, 12), train (nt, 12)) uint32: random_descriptors under a salt's XOR mask (distances unchanged) and
    train order (other indices, other first minima)"""
    if nq == 0 or nt == 0:
        rng = np.random.RandomState(77 + 1000 * nq + nt + salt)
        q, t = np.zeros((nq, 12), np.uint32), np.zeros((nt, 12), np.uint32)
        q[:, 4:] = rng.randint(0, 2 ** 32, (nq, 8), dtype=np.uint64)
        t[:, 4:] = rng.randint(0, 2 ** 32, (nt, 8), dtype=np.uint64)
        return q, t
    k1, k2 = random_descriptors(nq, nt)
    q, t = raw(k1).copy(), raw(k2).copy()
    if salt:
        rng = np.random.RandomState(salt)
        m = rng.randint(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
        q[:, 4:] ^= m
        t[:, 4:] ^= m
        t = t[rng.permutation(nt)]
    q[:, 0], t[:, 0] = np.arange(nq), np.arange(nt)  # pt.x: tells the records apart, never read by the matcher
    return q, t


class Batch:
    """nset1 query sets and nset2 train sets in the layout of gsh_orb_extract_batch_nostdlib: (nset, cap, 12) records and
    (nset) counts.  sizes: per set (nq, nt); the slots beyond a count are filled with the OTHER set's descriptors"""

    def __init__(self, sizes, nset1=None, nset2=None, cap1=None, cap2=None, salt=0):
        self.n = len(sizes)
        nset1, nset2 = nset1 or self.n, nset2 or self.n
        cap1 = cap1 or max(1, max(s[0] for s in sizes))
        cap2 = cap2 or max(1, max(s[1] for s in sizes))
        self.k1, self.k2 = np.zeros((nset1, cap1, 12), np.uint32), np.zeros((nset2, cap2, 12), np.uint32)
        self.n1, self.n2 = np.zeros(nset1, np.uint32), np.zeros(nset2, np.uint32)
        for p, (nq, nt) in enumerate(sizes):
            a, b = p if nset1 > 1 else 0, p if nset2 > 1 else 0
            if (nset1 == 1 and p) or (nset2 == 1 and p):  # a shared set was made with pair 0: only the other side is new
                q0, t0 = pair(nq, nt, salt)
                q, t = (q0, self._shuffled(t0, p)) if nset1 == 1 else (self._shuffled(q0, p), t0)
            else:
                q, t = pair(nq, nt, salt + 13 * p)
            if nset1 > 1 or p == 0:
                self.k1[a, :nq], self.n1[a] = q, nq
                self._fill(self.k1[a, nq:], t)
            if nset2 > 1 or p == 0:
                self.k2[b, :nt], self.n2[b] = t, nt
                self._fill(self.k2[b, nt:], q)

    @staticmethod
    def _shuffled(r, p):
        return r[np.random.RandomState(500 + p).permutation(len(r))]

    @staticmethod
    def _fill(slots, other):
        if len(slots) and len(other):
            slots[:] = other[np.arange(len(slots)) % len(other)]
        elif len(slots):
            slots[:, 4:] = 0x0F0F0F0F

    def sets(self, p):
        """the records pair p matches: (queries, train)"""
        a, b = p if len(self.k1) > 1 else 0, p if len(self.k2) > 1 else 0
        return self.k1[a], int(self.n1[a]), self.k2[b], int(self.n2[b])


_EXPECTED = {}


def expected(oracles, key, sets, mm, md):
    """per pair the oracle's records as (h, 3) uint32, computed once per case and shared by every back end and schedule"""
    key = (key, mm, md)
    if key not in _EXPECTED:
        want = []
        for o in oracles:
            per_pair = []
            for (k1, nq, k2, nt) in sets:
                m = o.match_orb(records(k1)[:nq], records(k2)[:nt], mm, md) if mm else np.zeros(0, np.uint32)
                per_pair.append(np.ascontiguousarray(m).view(np.uint32).reshape(-1, 3))
            want.append(per_pair)
        for w in want[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(w, want[0])), "the oracles disagree on %s" % (key,)
        _EXPECTED[key] = want[0]
    return _EXPECTED[key]


def typed(gd, shape):
    """a Guarded buffer's payload as uint32 (numpy) / int32 (torch) of `shape`"""
    v = gd.view((gd.n,))
    if isinstance(v, np.ndarray):
        return v.view(np.uint32).reshape(shape)
    import torch
    return v.view(torch.int32).reshape(shape)


def run(g, mem, oracles, key, b, mm, md, what, null_counts=False, counts1=None, counts2=None, moff=0, alias=False):
    """one gsh_match_orb_batch call on guarded buffers against the oracle -> (counts, matches (n, mm, 3)) as the library gave them.
    counts1 / counts2: the device-side counts to pass where they differ from the batch's (clamping); alias: k2 IS k1"""
    n = b.n
    clamp = lambda c, cap: np.minimum(c, cap)
    n1 = None if null_counts else np.asarray(b.n1 if counts1 is None else counts1, np.uint32)
    n2 = None if null_counts else np.asarray(b.n2 if counts2 is None else counts2, np.uint32)
    sets = []
    for p in range(n):
        k1, nq, k2, nt = b.sets(p)
        a, c = p if len(b.k1) > 1 else 0, p if len(b.k2) > 1 else 0
        nq = len(k1) if n1 is None else int(clamp(n1[a], len(k1)))
        nt = len(k2) if n2 is None else int(clamp(n2[c], len(k2)))
        sets.append((k1, nq, k2, nt))
    want = expected(oracles, key, sets, mm, md)
    g1 = Guarded(mem, b.k1.view(np.uint8))
    g2 = g1 if alias else Guarded(mem, b.k2.view(np.uint8), off=4)
    d1, d2 = typed(g1, b.k1.shape), typed(g2, b.k2.shape)
    c1 = None if n1 is None else Guarded(mem, n1.view(np.uint8))
    c2 = c1 if alias else (None if n2 is None else Guarded(mem, n2.view(np.uint8)))
    out = Guarded(mem, np.full(n * max(mm, 1) * 12, FILL, np.uint8), off=moff)
    cnt = Guarded(mem, np.full(n * 4, FILL, np.uint8))
    v1 = d1 if len(b.k1) > 1 else d1[0]  # one set: also the (cap, 12) form of the wrapper
    if mm:
        g.match_orb_batch(v1, None if c1 is None else typed(c1, (len(b.k1),)), d2, None if c2 is None else typed(c2, (len(b.k2),)),
                          typed(out, (n, mm, 3)), typed(cnt, (n,)), md)
    else:  # a (n, 0, 3) tensor has no address: the C entry with the buffer's own
        from grayskull_amd import _ptr
        g.c.gsh_match_orb_batch(_ptr(d1), b.k1.shape[1], None if c1 is None else _ptr(typed(c1, (len(b.k1),))), len(b.k1),
                                _ptr(d2), b.k2.shape[1], None if c2 is None else _ptr(typed(c2, (len(b.k2),))), len(b.k2),
                                n, _ptr(typed(out, (n, 1, 3))), _ptr(typed(cnt, (n,))), 0, md)
    counts = cnt.payload(what).view(np.uint32)
    got = out.payload(what).reshape(n, max(mm, 1) * 12)
    for p in range(n):
        h = len(want[p])
        assert counts[p] == h, "%s: pair %d of %d x %d: %d matches, expected %d" % (what, p, sets[p][1], sets[p][3], counts[p], h)
        rec = got[p, :h * 12].view(np.uint32).reshape(h, 3)
        bad = np.argwhere((rec != want[p]).any(axis=1))
        assert bad.size == 0, "%s: pair %d: %d records differ, first %d: got %s, expected %s" % (
            what, p, len(bad), bad[0, 0], rec[bad[0, 0]], want[p][bad[0, 0]])
        assert (got[p, h * 12:] == FILL).all(), "%s: pair %d: records at and beyond its count were written" % (what, p)
    assert np.array_equal(g1.payload(what), b.k1.view(np.uint8).reshape(-1)), what + ": k1 was written"
    assert np.array_equal(g2.payload(what), (b.k1 if alias else b.k2).view(np.uint8).reshape(-1)), what + ": k2 was written"
    for c, a in ((c1, n1), (c2, n2)):
        assert c is None or np.array_equal(c.payload(what).view(np.uint32), a), what + ": the counts were written"
    return counts, [w.copy() for w in want]


# ---- the cases -----------------------------------------------------------------------------------------------------------
CROSSED = ((1, 1), (63, T - 1), (64, T), (65, T + 1), (129, 2 * T + 1), (0, T), (64, 0), (65, 1), (1, S * T), (63, 2 * S * T + 1),
           (129, S * (T - 1)))


def check_sizes_in_one_batch(g, mem, oracles):
    """1: eleven pairs of different sizes behind device-side counts, every slot beyond a count an exact partner: the tile
    edges T - 1, T, T + 1, 2 T + 1, slices of exactly T - 1, T and 2 T + 1 descriptors (S (T - 1), S T and 2 S T + 1 train
    descriptors), a pair without queries and one without train descriptors between full pairs"""
    assert plan(S * T) == (T, S, 1) and plan(S * (T - 1)) == (T - 1, S, 1) and plan(2 * S * T + 1) == (2 * T + 1, S, 3)
    b = Batch(CROSSED, salt=1)
    counts, _ = run(g, mem, oracles, "crossed", b, 200, 60.0, "crossed sizes")
    assert counts[5] == 0 and counts[6] == 0 and counts[2] > 0 and counts[10] > 0


def check_two_chunks_of_queries(g, mem, oracles):
    """2: 2049 queries (33 mask words, two compaction chunks) against S T + 1 train descriptors (two tiles per slice, the
    second with one descriptor); one pair, NULL counts, and the cap falls inside the second chunk's first word"""
    assert plan(S * T + 1) == (T + 1, S, 2)
    b = Batch(((2049, S * T + 1),), salt=2)
    counts, want = run(g, mem, oracles, "2049", b, 2049, 60.0, "2049 x 1025", null_counts=True)
    h = int(counts[0])
    assert h > 100 and want[0][-1][0] >= 2048  # accepted queries in both chunks
    below = int((want[0][:, 0] < 2048).sum())
    run(g, mem, oracles, "2049", b, below + 1, 60.0, "2049 x 1025, cap one record into the second chunk", null_counts=True)


def check_set_sharing(g, mem, oracles):
    """3: one query set against n train sets, n against one, n against n, n = 1, and k1 aliasing k2 (every set against itself:
    every accepted query is matched to its own index at distance 0)"""
    sizes = ((70, 130),) * 3
    run(g, mem, oracles, "1:n", Batch(sizes, nset1=1, salt=3), 70, 60.0, "one query set, three train sets")
    run(g, mem, oracles, "n:1", Batch(sizes, nset2=1, salt=4), 70, 60.0, "three query sets, one train set")
    run(g, mem, oracles, "n:n", Batch(sizes, salt=5), 70, 60.0, "three against three")
    run(g, mem, oracles, "n=1", Batch(((65, 65),), salt=6), 65, 60.0, "one pair")
    b = Batch(((70, 70), (70, 70), (33, 33)), salt=7)
    b.k2, b.n2 = b.k1, b.n1
    counts, want = run(g, mem, oracles, "alias", b, 70, 60.0, "k1 aliasing k2", alias=True)
    assert all((w[:, 0] == w[:, 1]).all() and (w[:, 2] == 0).all() for w in want) and counts[2] > 0


def check_device_counts(g, mem, oracles):
    """4: counts below cap (slots beyond them hold exact partners), counts above cap (clamped), NULL counts (every slot counts)"""
    sizes = ((40, 90), (66, 50), (20, 129))
    b = Batch(sizes, cap1=70, cap2=140, salt=8)
    below, _ = run(g, mem, oracles, "below", b, 70, 60.0, "counts below cap")
    over1, over2 = np.array([75, 0xFFFFFFFF, 71], np.uint32), np.array([141, 140, 0x80000000], np.uint32)
    above, _ = run(g, mem, oracles, "above", b, 70, 60.0, "counts above cap", counts1=over1, counts2=over2)
    null, _ = run(g, mem, oracles, "above", b, 70, 60.0, "NULL counts", null_counts=True)
    assert np.array_equal(above, null) and not np.array_equal(above, below)


def check_match_cap(g, mem, oracles):
    """5: max_matches = 1, H - 1, H, H + 1 for the H accepted queries of pair 0; 0; and a matches pointer that is only
    4-byte aligned"""
    b = Batch(((129, 129), (100, 129)), salt=9)
    counts, _ = run(g, mem, oracles, "cap", b, 129, 256.0, "no cap")
    h = int(counts[0])
    assert 3 < h < 129
    for mm in (1, h - 1, h, h + 1):
        c, _ = run(g, mem, oracles, "cap", b, mm, 256.0, "max_matches = %d, H = %d" % (mm, h), moff=4 if mm == h - 1 else 0)
        assert c[0] == min(mm, h)
    c, _ = run(g, mem, oracles, "cap", b, 0, 256.0, "max_matches = 0")
    assert not c.any()


def check_distance_limits(g, mem, oracles):
    """6: max_distance 256, 60, 2 and -1 (no match at all); 59.5 starts the search at a value that is no integer"""
    b = Batch(((65, 129), (64, 65)), salt=10)
    seen = []
    for md in (256.0, 60.0, 2.0, -1.0, 59.5, 0.0):
        c, _ = run(g, mem, oracles, "dist", b, 65, md, "max_distance = %g" % md)
        seen.append(int(c.sum()))
    assert seen[0] >= seen[1] > seen[2] > 0 and seen[3] == 0 and seen[5] > 0


def check_launch_split(g, mem, oracles):
    """7: GSH_TUNE_FRAMES_PER_LAUNCH = 2 with five pairs: launches of 2, 2 and 1 pairs give what one launch gives, also with
    a shared query set"""
    sizes = ((30, 70), (64, 64), (65, 10), (5, 129), (66, 66))
    whole, _ = run(g, mem, oracles, "split", Batch(sizes, salt=11), 66, 60.0, "five pairs, one launch")
    g.tune(8, 2)
    try:
        parts, _ = run(g, mem, oracles, "split", Batch(sizes, salt=11), 66, 60.0, "five pairs, two per launch")
        run(g, mem, oracles, "split 1:n", Batch(((66, 66),) * 5, nset1=1, salt=12), 66, 60.0, "one query set, two pairs per launch")
    finally:
        g.tune(8, 0)
    assert np.array_equal(whole, parts)


def check_nothing_for_no_pairs(g, mem, oracles):
    """8: n = 0 launches nothing and checks nothing (the NULL and zero arguments would abort)"""
    a = mem.zeros((2, 9, 12), np.uint32, fill=3)
    m = mem.zeros((2, 4, 3), np.uint32, fill=0x5A5A5A5A)
    c = mem.zeros((2,), np.uint32, fill=0x5A5A5A5A)
    g.match_orb_batch(a, None, a, None, m[0:0], c[0:0], 60.0)
    g.c.gsh_match_orb_batch(None, 0, None, 7, None, 0, None, 9, 0, None, None, 5, 60.0)
    sync(mem)
    assert (np.asarray(mem.get(m, np.uint32)) == 0x5A5A5A5A).all() and (np.asarray(mem.get(c, np.uint32)) == 0x5A5A5A5A).all()


ALL_CHECKS = (check_sizes_in_one_batch, check_two_chunks_of_queries, check_set_sharing, check_device_counts, check_match_cap,
              check_distance_limits, check_launch_split, check_nothing_for_no_pairs)
