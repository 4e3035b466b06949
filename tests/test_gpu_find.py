"""shafa_hipd_find_dev (csrc/find.hip) and shafa.find against Python on the host: i = data.find(pat); while i >= 0: ...;
i = data.find(pat, i + 1).  For a chain the oracle runs over the concatenated bytes, maps each start back to (region, offset)
and drops the starts in context regions.  d_count, d_total and d_hits are compared exactly; nothing is compared with device
code.

The shapes are the smallest at which the kernels can go wrong: a lane is 32 bytes, a wave 2048, a tile 8192, the halo at
most 255.  Every region lies at one of the alignments 0, 1, 15, 16, 17 in a buffer whose guard and slack bytes are copies of
the pattern, so a read in front of a region or behind d_in_n shows up as a wrong count.  The background is seeded random bytes
over four symbols, the patterns are drawn from the same four: prefixes of the pattern occur often and the filter on the first
four bytes passes many false candidates.  The full range of alignments, 0 .. 15 at every region size, is
test_gpu_every_alignment.py's."""
import bisect

import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ALIGN = (0, 1, 15, 16, 17)
GUARD = -0x0123456789ABCDEF
ABC = np.frombuffer(b"abcd", dtype=np.uint8)


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(rng, n):
    return ABC[rng.integers(0, 4, n)].tobytes()


def _oracle(regions, flags, pat):
    """-> (matches charged to each region, [(region, offset)] in order)"""
    counts, hits, i = [0] * len(regions), [], 0
    while i < len(regions):
        j = i
        while flags[j] & 1:
            j += 1
        data = b"".join(regions[i:j + 1])
        ends = list(np.cumsum([len(r) for r in regions[i:j + 1]]))
        k = data.find(pat)
        while k >= 0:
            r = bisect.bisect_right(ends, k)                         # skips the empty regions
            if not flags[i + r] & 2:
                counts[i + r] += 1
                hits.append((i + r, k - (ends[r] - len(regions[i + r]))))
            k = data.find(pat, k + 1)
        i = j + 1
    return counts, hits


def _place(regions, pat, slack, aligns=ALIGN):
    """The regions in one host buffer made of copies of the pattern, a copy ending right in front of each region and one
    starting right behind its bytes (its slack, then its guard); region i at alignment aligns[i % len(aligns)] (ALIGN[i % 5]
    unless the caller brings its own) -> (buffer, offsets, caps)"""
    m = len(pat)
    off, cap, pos = [], [], 0
    for i, r in enumerate(regions):
        pos = (pos + m + 32 + 255) // 256 * 256 + 32 * (i % 3) + aligns[i % len(aligns)]
        off.append(pos)
        cap.append(len(r) + (slack[i] if slack else 0))
        pos += cap[-1]
    total = pos + m + 64
    buf = bytearray((pat * (total // m + 1))[:total])
    for o, r in zip(off, regions):
        buf[o - m:o] = pat
        buf[o:o + len(r)] = r
        buf[o + len(r):o + len(r) + m] = pat
    return np.frombuffer(bytes(buf), dtype=np.uint8), off, cap


class _Run:
    """one find_dev call on real regions -> counts, total, hits (the whole array, guard values behind), per-block codes;
    `addr`: the device address of every region"""

    def __init__(self, shafa, regions, flags, pat, max_hits=None, slack=None, over=(), pos=None, append=None, null_hits=False,
                 aligns=ALIGN):
        nb = len(regions)
        buf, self.off, self.cap = _place(regions, pat, slack, aligns)
        self.pos = pos if pos is not None else [(i << 34) + 7 * i for i in range(nb)]
        sizes = [c + 1 + i if i in over else len(r) for i, (r, c) in enumerate(zip(regions, self.cap))]
        self.regions = [b"" if i in over else r for i, r in enumerate(regions)]      # what the call may look at
        self.flags = list(flags) if flags is not None else [0] * nb
        self.counts, self.hits = _oracle(self.regions, self.flags, pat)
        self.want = [self.pos[r] + o for r, o in self.hits]
        if append is not None:
            max_hits = append.max_hits
        elif max_hits is None:
            max_hits = len(self.want) + 3
        self.max_hits = max_hits
        self._device(shafa, buf, sizes, flags, pat, append, null_hits)

    def _device(self, shafa, buf, sizes, flags, pat, append, null_hits):
        import torch
        nb, max_hits = len(sizes), self.max_hits
        d_in = torch.from_numpy(buf.copy()).to(_dev())
        self.addr = [d_in.data_ptr() + o for o in self.off]
        d_n = torch.tensor(sizes, dtype=torch.int64).to(_dev())
        if append is None:
            self.d_hits = torch.full((max_hits + 8,), GUARD, dtype=torch.int64, device=_dev())
            self.d_total = torch.zeros(1, dtype=torch.int64, device=_dev())
            self.t0 = 0
        else:
            self.d_hits, self.d_total, self.t0 = append.d_hits, append.d_total, append.total
        d_count = torch.full((nb + 1,), -1, dtype=torch.int64, device=_dev())
        bt = shafa.Batch(nb, 1 << 20)
        st = torch.cuda.Stream(device=_dev())
        try:
            bt.find_dev(st, d_in, self.off, self.cap, d_n, flags, self.pos, pat, max_hits, None if null_hits else self.d_hits,
                        d_count, self.d_total)
            self.rc, self.errs = bt.finish(st, nb, raise_on_error=False)
        finally:
            bt.close()
        got = d_count.cpu().tolist()
        assert got[nb] == -1
        self.got_counts = got[:nb]
        self.total = int(self.d_total.cpu()[0])
        self.got_hits = self.d_hits.cpu().tolist()

    def check(self, what=""):
        assert self.got_counts == self.counts, (what, [(i, g, w) for i, (g, w) in enumerate(zip(self.got_counts, self.counts))
                                                       if g != w][:10])
        assert self.total == self.t0 + len(self.want), (what, self.total, self.t0, len(self.want))
        k0, k1 = min(self.t0, self.max_hits), min(self.total, self.max_hits)
        assert self.got_hits[k0:k1] == self.want[:k1 - k0], what
        assert all(v == GUARD for v in self.got_hits[k1:]), what     # nothing behind the total, nothing behind max_hits
        return self


# ---------------------------------------------------------------- single regions
SIZES = lambda m: sorted({0, 1, max(m - 1, 0), m, m + 1, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 33})
BORDERS = (32, 2048, 8192, 16384)


def _planted(rng, n, pat, starts, miss=False):
    """n random bytes with the pattern (or, miss: the pattern with its last byte wrong) written at these starts"""
    m = len(pat)
    x = bytearray(_rand(rng, n))
    w = pat[:-1] + bytes([pat[-1] ^ 0x20]) if miss else pat
    for s in starts:
        if 0 <= s and s + m <= n:
            x[s:s + m] = w
    return bytes(x)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 31, 32, 33, 64, 255, 256])
def test_single_regions(shafa, m):
    rng = _rng(1000 + m)
    pat = _rand(rng, m)
    regions = []
    for n in SIZES(m):
        for a in range(len(ALIGN)):                                  # region i lies at ALIGN[i % 5]: every size at every one
            starts = [0, n - m] if a % 2 == 0 else [0, n - m] + [b - m + a for b in BORDERS]
            regions.append(_planted(rng, n, pat, starts, miss=a == 3))
    # a match, and a near-miss with only the last byte wrong, at every start in [B - m, B + 1] of every border B
    for B in BORDERS:
        for s in range(max(B - m, 0), B + 2):
            n = max(s + m, B + 1) + (s % 7)
            regions.append(_planted(rng, n, pat, [s]))
            if m <= 33 or s % 8 == 0 or s >= B - 1:
                regions.append(_planted(rng, n, pat, [s], miss=True))
    slack = [(7 * i) % 23 for i in range(len(regions))]
    r = _Run(shafa, regions, None, pat, slack=slack).check(f"m={m}")
    assert r.rc == 0 and not any(r.errs)
    assert sum(r.counts) >= len(regions) // 3                        # the planted ones are there
    flags = [0] * len(regions)                                       # the same with an explicit array of zero flags
    _Run(shafa, regions[:40], flags[:40], pat, slack=slack[:40]).check(f"m={m}, zero flags")


# ---------------------------------------------------------------- overlaps
def test_overlapping_matches_all_count(shafa):
    a = b"a" * 8200
    for pat, want in ((b"a", 8200), (b"aaaa", 8197), (b"a" * 256, 8200 - 255)):
        r = _Run(shafa, [a, a[:10], b"a" * 255 + b"b" + b"a" * 300], None, pat).check(pat[:8])
        assert r.counts[0] == want and r.counts[1] == max(0, 10 - len(pat) + 1)
    ab = b"ab" * 4200
    r = _Run(shafa, [ab, ab[1:]], None, b"abab").check("abab")
    assert r.counts == [4199, 4198]
    assert [h - r.pos[0] for h in r.want[:3]] == [0, 2, 4]
    # the dense case: every position a candidate and a match, more than one tile, an odd tail
    r = _Run(shafa, [b"c" * (2 * 8192 + 77)], None, b"c").check("dense")
    assert r.counts == [2 * 8192 + 77]


# ---------------------------------------------------------------- chains
def _chain(n):
    return [1] * (n - 1) + [0]


def test_chain_over_an_empty_region(shafa):
    rng = _rng(7)
    pat = b"dcbadcb"
    sizes = [5, 0, 1, 3, 8192, 2]
    whole = bytearray(_rand(rng, sum(sizes)).replace(b"dcb", b"aaa"))
    whole[2:9] = pat                                                  # bytes 2 .. 8: regions 0, (1,) 2 and 3
    whole[8197:8201] = pat[:4]                                        # a prefix that runs out of bytes at the chain's end
    cuts = [0] + list(np.cumsum(sizes))
    regions = [bytes(whole[a:z]) for a, z in zip(cuts, cuts[1:])]
    r = _Run(shafa, regions, _chain(6), pat).check("chained")
    assert r.counts == [1, 0, 0, 0, 0, 0] and r.want == [r.pos[0] + 2]
    # without NEXT a region is its own chain
    r = _Run(shafa, regions, None, pat).check("unchained")
    assert sum(r.counts) == 0
    # two chains: the cut goes through the match
    r = _Run(shafa, regions, [1, 1, 0, 1, 1, 0], pat).check("two chains")
    assert sum(r.counts) == 0
    # one-byte and two-byte patterns over the same regions
    for p in (bytes(whole[4:5]), bytes(whole[4:6]), bytes(whole[5:7]), bytes(whole[8:10])):
        assert sum(_Run(shafa, regions, _chain(6), p).check(p).counts) >= 1


@pytest.mark.parametrize("nreg,size", [(300, 100), (40, 1)])
def test_long_chains(shafa, nreg, size):
    rng = _rng(nreg)
    whole = _rand(rng, nreg * size)
    regions = [whole[i * size:(i + 1) * size] for i in range(nreg)]
    pats = [whole[size - 5:size - 5 + m] for m in (1, 2, 7, 100, 101, 201, 256)] if size > 1 else \
        [whole[10:11], whole[10:12], whole[10:15], whole[1:40], whole[:40], whole[:40] + b"a"]
    for pat in pats:
        r = _Run(shafa, regions, _chain(nreg), pat).check(("chained", len(pat)))
        # the oracle on the whole: the same starts
        k, starts = whole.find(pat), []
        while k >= 0:
            starts.append(k)
            k = whole.find(pat, k + 1)
        assert [(reg * size + o) for reg, o in r.hits] == starts and (starts or len(pat) > 39)
        inner = _Run(shafa, regions, None, pat).check(("unchained", len(pat)))
        assert inner.hits == [(reg, o) for reg, o in r.hits if o + len(pat) <= size]
    # chains of three regions: the flags cut
    flags = [0 if i % 3 == 2 else 1 for i in range(nreg)]
    flags[-1] = 0
    for pat in pats[:4]:
        _Run(shafa, regions, flags, pat).check(("threes", len(pat)))


def test_region_past_its_capacity_counts_as_empty(shafa):
    rng = _rng(3)
    pat = b"abcab"
    x = bytearray(_rand(rng, 600).replace(b"abc", b"ddd"))
    x[98:103] = pat                                                   # over regions 0 | 1
    x[150:155] = pat                                                  # inside region 1
    x[197:202] = pat                                                  # over regions 1 | 2 (| 3: region 2 is 3 bytes)
    x[196:197] = b"d"
    cuts = [0, 100, 200, 203, 400, 600]
    regions = [bytes(x[a:z]) for a, z in zip(cuts, cuts[1:])]
    r = _Run(shafa, regions, _chain(5), pat).check("all good")
    assert r.counts[:2] == [1, 2] and not any(r.errs)
    for bad in (1, 2, 4, 0):
        r = _Run(shafa, regions, _chain(5), pat, over=(bad,), slack=[3] * 5).check(("bad", bad))
        assert r.errs == [shafa.OUTSIDE_MODULE if i == bad else 0 for i in range(5)] and r.rc == shafa.OUTSIDE_MODULE
        assert r.got_counts[bad] == 0
    # with region 2 gone, regions 1 and 3 are neighbours: the oracle's bytes are joined the same way
    y = regions[1][:97] + b"abc" + b"ab" + regions[3][2:]
    r = _Run(shafa, [regions[0], y[:100], b"zzz", y[100:]], _chain(4), pat, over=(2,)).check("joined over a bad region")
    assert (1, 97) in r.hits


def test_context_regions(shafa):
    m, pat = 5, b"ababa"
    rng = _rng(9)
    for cl in (0, 1, m - 1):
        for hl in (0, 1, m - 1):
            for carry, head in ((b"ababa"[-cl:] if cl else b"", b"babab"[:hl] if cl % 2 == 0 else b"ababa"[:hl]),
                                (_rand(rng, cl), _rand(rng, hl))):
                r = _Run(shafa, [carry, head], [1, 2], pat, pos=[1000 - cl, 1000]).check((cl, hl))
                assert r.got_counts[1] == 0
                if cl == hl == m - 1 and carry == b"baba":
                    assert r.want == [997, 999]                        # both start in the carry; a third would not fit
    # a context region in mid-chain supplies bytes and reports nothing; one with matches of its own
    regions = [b"xxaba", b"bababab", b"ababa"]
    r = _Run(shafa, regions, [1, 3, 0], pat).check("mid-chain context")
    assert r.counts[1] == 0 and r.counts[0] >= 1 and r.counts[2] == 1
    assert _Run(shafa, regions, [1, 1, 0], pat).check("no context").counts[1] >= 2
    big = b"ab" * 6000                                                # a context region of more than a tile
    r = _Run(shafa, [big, big, big], [0, 2, 0], b"abab").check("context tile")
    assert r.counts == [5999, 0, 5999]


# ---------------------------------------------------------------- capacity and appending
def _busy(rng):
    pat = b"abca"
    regions = [_planted(rng, n, pat, range(5, n, 97)) for n in (9000, 300, 20000, 4)]
    return regions, pat


def test_max_hits_keeps_the_first_in_order(shafa):
    regions, pat = _busy(_rng(21))
    full = _Run(shafa, regions, [1, 0, 1, 0], pat).check("all")
    total = len(full.want)
    assert total > 300
    for mh in (1, 2, 63, 64, 65, 92, 93, 94, total - 1, total, total + 1):
        r = _Run(shafa, regions, [1, 0, 1, 0], pat, max_hits=mh).check(mh)
        assert r.total == total and r.got_hits[:min(mh, total)] == full.want[:mh]
    r = _Run(shafa, regions, [1, 0, 1, 0], pat, max_hits=0, null_hits=True).check("counts only")
    assert r.total == total and r.got_counts == full.counts


def test_calls_append(shafa):
    regions, pat = _busy(_rng(22))
    a = _Run(shafa, regions[:2], [1, 0], pat, max_hits=400).check("first")
    b = _Run(shafa, regions[2:], [1, 0], pat, append=a, pos=[1 << 40, (1 << 40) + 20000]).check("second")
    assert b.total == len(a.want) + len(b.want) and b.got_hits[:len(a.want)] == a.want
    c = _Run(shafa, regions, None, pat, append=b).check("third, past max_hits")
    assert c.total > 400 and c.got_hits[:b.total] == b.got_hits[:b.total]


def test_same_call_same_bytes(shafa):
    rng = _rng(23)
    whole = _planted(rng, 70000, b"dd", range(0, 70000, 5))
    regions = [whole[:33333], whole[33333:40000], whole[40000:]]
    a = _Run(shafa, regions, _chain(3), b"dd").check()
    b = _Run(shafa, regions, _chain(3), b"dd").check()
    assert a.got_hits == b.got_hits and len(a.want) > 14000


# ---------------------------------------------------------------- tiles numbered from the capacities
def test_more_tiles_than_workgroups(shafa):
    """three regions with 64 MiB of capacity each, in a buffer that really is that large: 24576 tiles, two to a workgroup"""
    import torch
    CAP, N = 1 << 26, 20000
    rng = _rng(31)
    pat = b"abcdabc"
    d_in = torch.empty(3 * CAP + 64, dtype=torch.uint8, device=_dev())
    off = [3, CAP + 1, 2 * CAP + 18]
    regions = [_planted(rng, N, pat, [0, 8190, 16380, N - 7, 5000 + i]) for i in range(3)]
    for o, r in zip(off, regions):
        d_in[o:o + N + 64].copy_(torch.frombuffer(bytearray(r + (pat * 10)[:64]), dtype=torch.uint8))
    d_n = torch.tensor([N] * 3, dtype=torch.int64).to(_dev())
    d_hits = torch.full((1000,), GUARD, dtype=torch.int64, device=_dev())
    d_count = torch.zeros(3, dtype=torch.int64, device=_dev())
    d_total = torch.zeros(1, dtype=torch.int64, device=_dev())
    bt = shafa.Batch(3, CAP)
    st = torch.cuda.Stream(device=_dev())
    try:
        bt.find_dev(st, d_in, off, [CAP - 32] * 3, d_n, None, [0, 1 << 30, 1 << 31], pat, 1000, d_hits, d_count, d_total)
        rc, errs = bt.finish(st, 3, raise_on_error=False)
    finally:
        bt.close()
    counts, hits = _oracle(regions, [0] * 3, pat)
    assert rc == 0 and d_count.cpu().tolist() == counts and int(d_total.cpu()[0]) == len(hits) >= 15
    got = d_hits.cpu().tolist()
    assert got[:len(hits)] == [(0, 1 << 30, 1 << 31)[r] + o for r, o in hits] and set(got[len(hits):]) == {GUARD}


# ---------------------------------------------------------------- the find driver
def _all(data, pat):
    k, out = data.find(pat), []
    while k >= 0:
        out.append(k)
        k = data.find(pat, k + 1)
    return out


def _found(shafa, got, data, pat, max_hits=65536):
    want = _all(data, pat)
    assert isinstance(got, shafa.Found) and type(got.count) is int and got.count == len(want), (got.count, len(want))
    assert got.positions.dtype == np.int64 and got.positions.tolist() == want[:max_hits]
    assert got.size == len(data)
    return want


def test_find_pieces(shafa):
    import torch
    rng = _rng(41)
    n = (1 << 20) + 77
    pat = b"dcbaabcdd"
    seams = sorted(s for piece in (8192, 40000, 1 << 20) for s in range(piece, n, piece))
    starts = [0]
    for i, s in enumerate(seams):                                      # over the seam by 8, 5 or 1 bytes, or ending at it
        if s - 9 >= starts[-1] + 32:
            starts.append(s - (1, 4, 8, 9)[i % 4])
    starts.append(n - len(pat))
    data = _planted(rng, n, pat, starts)
    base = torch.from_numpy(np.frombuffer(b"xyz" + data, dtype=np.uint8).copy()).to(_dev())
    d_in = base[3:]
    assert d_in.data_ptr() % 16 == 3
    want = None
    for piece in (8192, 40000, 1 << 20, None):
        want = _found(shafa, shafa.find(d_in, pat, _piece=piece), data, pat)
        assert len(want) >= 100
    assert set(starts) <= set(want) and {40000 - s for s in starts} & {1, 4, 8} and (1 << 20) - 9 < starts[-2] < 1 << 20
    for mh in (0, 1, 5):
        _found(shafa, shafa.find(d_in, pat, max_hits=mh, _piece=40000), data, pat, mh)
    _found(shafa, shafa.find(d_in, b"b", _piece=40000), data, b"b")                      # more matches than max_hits
    _found(shafa, shafa.find(d_in, bytearray(b"ab"), max_hits=1 << 20, _piece=8192), data, b"ab", 1 << 20)
    _found(shafa, shafa.find(d_in[:0], pat), b"", pat)


def test_find_segments(shafa):
    import torch
    rng = _rng(42)
    pat = b"abcab"
    sizes = [0, 1, 5000, 0, 4, 5, 9000, 1, 20000]
    segs = [bytearray(_planted(rng, n, pat, range(3, n, 501))) for n in sizes]
    segs[2][-2:] = b"ab"                                               # "ab" | (empty) | "cab.": straddles, not reported
    segs[4][:] = b"cabc"
    segs[5][:] = pat
    segs[6][-3:] = b"abc"                                              # "abc" | "a" | "b...": over a one-byte segment
    segs[7][:] = b"a"
    segs[8][:1] = b"b"
    data = b"".join(bytes(s) for s in segs)
    assert len(_all(data, pat)) > sum(len(_all(bytes(s), pat)) for s in segs)      # the straddling ones exist
    d_in = torch.from_numpy(np.frombuffer(b"q" + data + b"tail", dtype=np.uint8).copy()).to(_dev())[1:]
    for kw in ({}, {"max_hits": 0}, {"max_hits": 1}, {"max_hits": 7, "_piece": 4096}, {"_piece": 8192}):
        got = shafa.find(d_in, pat, sizes=sizes, **kw)
        assert isinstance(got, list) and len(got) == len(sizes)
        for g, s in zip(got, segs):
            _found(shafa, g, bytes(s), pat, kw.get("max_hits", 65536))
    assert shafa.find(d_in, pat, sizes=[]) == []
    with pytest.raises(ValueError):
        shafa.find(d_in, pat, sizes=[d_in.numel(), 1])
    with pytest.raises(ValueError):
        shafa.find(d_in, pat, sizes=[-1])
    with pytest.raises(ValueError):
        shafa.find(d_in, pat, max_hits=-1)
    with pytest.raises(ValueError):
        shafa.find(d_in, b"")
    with pytest.raises(ValueError):
        shafa.find(d_in[::2], pat)
