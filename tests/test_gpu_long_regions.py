"""One region past 4 GiB in the entry points without a block-size limit (include/shafa_hip.h: "a file may exceed 4 GiB").

A region is LONG = 2^32 + 3 * 8192 + 5 bytes, the smallest shape that crosses the boundary and ends ragged, and starts LEAD = 2 GiB
into its own allocation, so that a position cut to 32 bits lands inside the allocation whether it is zero- or sign-extended and
shows as wrong bytes, not as a fault.  Data is made on the device; the expectations are plain torch statements (checked against
the suite's numpy references at small sizes in test_far_cpu.py) or follow by construction; nothing of 4 GiB crosses to the host.

    entry point                                   what crosses 2^32                      reference
    crc32_dev, shafa.crc32                        the region                             zlib.crc32 of the period, joined by crc_combine
    compare_dev                                   both operands                          the planted position
    find_dev, shafa.find                          the region, one match over the border  the planted positions
    split_planes_dev, merge_planes_dev (E = 1)    the element and the plane side         identity, one torch.equal
    split_planes_dev, merge_planes_dev (E = 4)    the element side                       torch transpose (a strided view)
    split_records_dev, merge_records_dev (W = 3)  the record side                        torch transpose (a strided view)
    split/merge_planes_grid_dev, hist_planes_grid_dev (E = 4, three lags)                torch_grid_z, torch_plane_hist
    pack_payloads, unpack_shaf, unpack_payloads   a .shaf of 64 x 64 MiB and two real blocks  the layout computed on the host, device slices
    sf_decode_dev, seek_index_dev, read_spans_dev the real blocks where they lie in the file  the oracle's bytes, the header's checkpoints
    compress_many, decompress_many                a first file of 2^32 bytes             the small files alone; the input

compress_tensors and read_ranges, which the 64-bit promise also matters to, have no run of their own here: compress_tensors is
split_planes_dev and the compress_many chain, read_ranges is read_spans_dev over the payload places unpack_shaf computed, and
each of those is above with its region or its places past 2^32; what the two drivers add is arithmetic on Python integers, and a
run through them would need another tensor or file set of 4 GiB and more.

At most three allocations of 6 GiB and two temporaries of 4 GiB are live at once in the kernel tests; the driver run comes first,
before those allocations exist.  test_peak_memory asserts the 24 GiB bound over the whole file."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 1 << 32
DELTA = 3 * 8192 + 5
LONG = G + DELTA
LEAD = 1 << 31                      # where a long region starts in its allocation
SLACK = 1 << 20
ALLOC = LEAD + LONG + SLACK
PERIOD = 12345677                   # odd: a position taken mod 2^32 reads another phase
FIND_PERIOD = 99991
FILL = 0xA5
GUARD = 64
LIMIT = 24 << 30
DEV = "cuda:0"
PATTERN = b"\xf0needle \x00\xff"


def al16(x):
    return (x + 15) // 16 * 16


def sign_extended(pos):
    """what a position becomes when its low 32 bits are taken as a signed int"""
    lo = pos & 0xFFFFFFFF
    return lo - G if lo >> 31 else lo


# ---------------------------------------------------------------- references (any device; test_far_cpu.py ties them to numpy)
def _gf2_times(mat, vec):
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1
        i += 1
    return s


def _gf2_square(mat):
    return [_gf2_times(mat, mat[n]) for n in range(32)]


def crc_combine(crc1, crc2, len2):
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B): the operator "append one zero bit" as a 32 x 32 matrix
    over GF(2), squared up to len2 bytes (Adler's crc32_combine); written here so that the reference is not the code under test"""
    if len2 <= 0:
        return crc1
    odd = [0xEDB88320] + [1 << n for n in range(31)]
    even = _gf2_square(odd)
    odd = _gf2_square(even)
    while True:
        even = _gf2_square(odd)
        if len2 & 1:
            crc1 = _gf2_times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = _gf2_square(even)
        if len2 & 1:
            crc1 = _gf2_times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def crc_of_span(period, start, length):
    """zlib.crc32 of `length` bytes from position `start` of the endless repetition of the bytes `period`"""
    p = len(period)
    head = period[start % p:][:length]
    crc, rest = zlib.crc32(head), length - len(head)
    if rest >= p:
        whole = zlib.crc32(period)
        shift = [crc_combine(1 << i, 0, p) for i in range(32)]             # "append p zero bytes" as a matrix
        for _ in range(rest // p):
            crc = _gf2_times(shift, crc) ^ whole
    if rest % p:
        crc = crc_combine(crc, zlib.crc32(period[:rest % p]), rest % p)
    return crc


def fill_repeat(region, period):
    """region (1-D uint8 tensor) = the tensor `period` repeated, cut at the region's end; no temporary of the region's size"""
    p, n = period.numel(), region.numel()
    k = n // p
    if k:
        region[:k * p].view(k, p).copy_(period.view(1, p).expand(k, p))
    region[k * p:].copy_(period[:n - k * p])


def random_period(seed, n, device):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(device)


def plant(region, pattern, positions, seed, period=FIND_PERIOD):
    """region = random bytes over the alphabet without pattern[0], with `pattern` (whose first byte occurs in it once) at
    `positions` and nowhere else"""
    import torch
    assert pattern[0] not in pattern[1:]
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randint(0, 255, (period,), generator=g, dtype=torch.uint8)
    q = q + (q >= pattern[0]).to(torch.uint8)
    fill_repeat(region, q.to(region.device))
    t = torch.tensor(list(pattern), dtype=torch.uint8, device=region.device)
    for at in positions:
        region[at:at + len(pattern)] = t


def torch_planes(el, k):
    """[k, n] view of the n elements of k bytes in the 1-D uint8 tensor `el`: row j is byte j of every element"""
    return el.view(-1, k).t()


def torch_grid_z(x, lags):
    """the zigzag fold of (1 - S^L1)(1 - S^L2)(1 - S^L3) x mod 2^(8 k) for a 1-D tensor of a signed integer dtype, written as
    taps: d[i] = sum over the subsets A of the lags of (-1)^|A| x[i - sum A]; x is only read, one result and one temporary"""
    import itertools
    n = x.numel()
    d = x.clone()
    for r in range(1, len(lags) + 1):
        for sub in itertools.combinations(lags, r):
            s = sum(sub)
            if s < n:
                if r % 2:
                    d[s:].sub_(x[:n - s])
                else:
                    d[s:].add_(x[:n - s])
    t = d >> (8 * x.element_size() - 1)                                    # arithmetic: 0 or -1
    d.mul_(2)
    d.bitwise_xor_(t)
    return d


def torch_plane_hist(z, chunk=1 << 26):
    """[k, 256] int64 counts of byte j of every element of the integer tensor z"""
    import torch
    k = z.element_size()
    b = z.view(torch.uint8).view(-1, k)
    out = torch.zeros(k, 256, dtype=torch.int64, device=z.device)
    for a in range(0, b.shape[0], chunk):
        for j in range(k):
            out[j] += torch.bincount(b[a:a + chunk, j].to(torch.int32), minlength=256)
    return out


# ---------------------------------------------------------------- the allocations
@pytest.fixture(scope="module", autouse=True)
def room():
    """every test of this file needs up to LIMIT bytes; the peak is counted from here (test_peak_memory)"""
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < LIMIT:
        pytest.skip(f"the long regions need {LIMIT} bytes of device memory, {free} are free")
    torch.cuda.reset_peak_memory_stats()
    print("device memory held when this file starts:", torch.cuda.memory_allocated())
    yield
    torch.cuda.empty_cache()


class Long:
    def __init__(self):
        import torch
        self.torch = torch
        self.a = torch.empty(ALLOC, dtype=torch.uint8, device=DEV)
        self.b = torch.empty(ALLOC, dtype=torch.uint8, device=DEV)
        assert self.a.data_ptr() % 16 == 0 and self.b.data_ptr() % 16 == 0

    def third(self):
        t = self.torch.empty(ALLOC, dtype=self.torch.uint8, device=DEV)
        t.fill_(FILL)
        return t

    def random_a(self, seed, nbytes=LONG):
        self.a.fill_(FILL)
        period = random_period(seed, PERIOD, DEV)
        fill_repeat(self.a[LEAD:LEAD + nbytes], period)
        return period


@pytest.fixture(scope="module")
def long():
    import torch
    x = Long()
    yield x
    x.a = x.b = None
    torch.cuda.empty_cache()


def call(shafa, nb, body):
    import torch
    st = torch.cuda.Stream(device=DEV)
    bt = shafa.Batch(nb, 1 << 20)
    try:
        torch.cuda.synchronize()
        body(bt, st)
        rc, errs = bt.finish(st, nb, raise_on_error=False)
    finally:
        bt.close()
    assert rc == 0 and errs == [0] * nb, (rc, errs)


def i64(v):
    import torch
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=DEV)


def untouched(t, lo, hi):
    """the GUARD bytes in front of t[lo:hi] and behind it still hold FILL"""
    return bool((t[lo - GUARD:lo] == FILL).all()) and bool((t[hi:hi + GUARD] == FILL).all())


# ---------------------------------------------------------------- one driver run end to end (before the 6 GiB allocations exist)
def test_compress_many_with_a_first_file_of_4_gib(shafa):
    """compress_many lays its blocks back to back in one buffer: behind a first file of 2^32 bytes of Zipf data every block of
    the five small files lies past byte 2^32.  Their file sets equal those of the small files compressed alone, and everything
    decodes to the input.  The small files are one block, one block of the block size, two blocks and four; none ends in a
    block of one byte, a block of one symbol, whose empty codes Module D refuses wherever it lies."""
    import torch
    small = [1024, 5000, 65536, 65536 + 1025, 200000]
    sizes = [G] + small
    st = torch.cuda.Stream(device=DEV)
    zt = torch.from_numpy(shafa.zipf_table(1.2)).to(DEV)

    def generate(first, n):
        """bytes [first, first + n) of the input: the generator is a function of the position"""
        t = torch.empty(n, dtype=torch.uint8, device=DEV)
        shafa.gen_bytes(st, 2026, first, t, n, zt)
        st.synchronize()
        return t

    d_in = generate(0, sum(sizes))
    sets = shafa.compress_many(d_in, sizes)
    print("peak after compress_many:", torch.cuda.max_memory_allocated())
    alone = shafa.compress_many(d_in[G:], small)
    assert all(isinstance(s, dict) for s in sets + alone)
    for f, (s, a) in enumerate(zip(sets[1:], alone)):
        assert sorted(s) == sorted(a) and all(torch.equal(s[k], a[k]) for k in s), f"small file {f}"
    del alone, d_in                                                       # the input is made again below, a piece at a time
    ent = []
    for s in sets:
        k = ".rle" if ".rle.shaf" in s else ""
        # copies: a file set's tensors are views of the group's worst-case pack regions, which would stay alive with them
        ent.append(dict(shaf=s[k + ".shaf"].clone(), cod=s[k + ".cod"].clone(), decode_rle=bool(k)))
    del sets, s
    torch.cuda.empty_cache()
    print("held before decompress_many:", torch.cuda.memory_allocated())
    back = shafa.decompress_many(ent)
    print("peak after decompress_many:", torch.cuda.max_memory_allocated())
    del ent
    torch.cuda.empty_cache()
    pos, piece = 0, 1 << 30
    for f, (n, r) in enumerate(zip(sizes, back)):
        assert isinstance(r, torch.Tensor) and r.numel() == n, f"file {f}: {r!r}"
        r = r.reshape(-1)
        for a in range(0, n, piece):
            m = min(piece, n - a)
            lead = (pos + a) % 16                                           # the generator starts at multiples of 16
            assert torch.equal(r[a:a + m], generate(pos + a - lead, m + lead)[lead:]), f"file {f} from byte {a}"
        pos += n


# ---------------------------------------------------------------- crc32
def test_crc32(long, shafa):
    import torch
    period = bytes(long.random_a(1).cpu().numpy())
    spans = [(0, LONG), (3, LONG - 3), (LONG - 100000, 100000), (G - 5, 77)]
    want = [crc_of_span(period, s, n) for s, n in spans]
    d_crc = torch.zeros(len(spans), dtype=torch.int32, device=DEV)
    ns = [n for _, n in spans]
    call(shafa, len(spans), lambda bt, st: bt.crc32_dev(st, long.a, [LEAD + s for s, _ in spans], ns, i64(ns), d_crc))
    got = [int(x) & 0xFFFFFFFF for x in d_crc.cpu().numpy()]
    print("crc32_dev", [hex(x) for x in got], [hex(x) for x in want])
    assert got == want
    assert shafa.crc32(long.a[LEAD:LEAD + LONG]) == want[0]
    assert shafa.crc32(long.a[LEAD + 3:LEAD + LONG], sizes=[LONG - 100003, 100000]) == [crc_of_span(period, 3, LONG - 100003), want[2]]


# ---------------------------------------------------------------- compare
def test_compare(long, shafa):
    import torch
    long.random_a(2)
    long.b.fill_(FILL)
    long.b[LEAD:LEAD + LONG].copy_(long.a[LEAD:LEAD + LONG])
    cases = [((), LONG), ((G + 12345,), G + 12345), ((LONG - 1,), LONG - 1), ((12345, G + 12345), 12345)]
    for flips, want in cases:
        for at in flips:
            long.b[LEAD + at] ^= 0x40
        d_first = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        call(shafa, 1, lambda bt, st: bt.compare_dev(st, long.b, [LEAD], [LONG], i64([LONG]), long.a, [LEAD], [LONG], d_first))
        for at in flips:
            long.b[LEAD + at] ^= 0x40
        assert int(d_first[0]) == want, (flips, int(d_first[0]))


# ---------------------------------------------------------------- find
# the pattern at 2^32 - 3 straddles the boundary and would overlap one at 2^32 (its first byte occurs in it once), so the two
# positions are planted in two data sets; each also holds the pattern at 7, just behind the boundary's match and at the very end
def planted_at(border, n):
    m = len(PATTERN)
    return {"straddles_2_32": (7, border - 3, border - 3 + m, n - m), "starts_at_2_32": (7, border - m, border, n - m)}


PLANTED = planted_at(G, LONG)


@pytest.mark.parametrize("max_hits", [65536, 2])
@pytest.mark.parametrize("where", sorted(PLANTED))
def test_find(long, shafa, where, max_hits):
    import torch
    HITS = PLANTED[where]
    long.a.fill_(FILL)
    plant(long.a[LEAD:LEAD + LONG], PATTERN, HITS, 3)
    d_hits = torch.full((max_hits,), -7, dtype=torch.int64, device=DEV)
    d_count, d_total = i64([-1]), i64([0])
    call(shafa, 1, lambda bt, st: bt.find_dev(st, long.a, [LEAD], [LONG], i64([LONG]), None, [1000], PATTERN, max_hits, d_hits, d_count,
                                              d_total))
    k = min(max_hits, len(HITS))
    assert int(d_count[0]) == len(HITS) and int(d_total[0]) == len(HITS)
    assert d_hits.cpu().tolist() == [1000 + h for h in HITS[:k]] + [-7] * (max_hits - k)
    found = shafa.find(long.a[LEAD:LEAD + LONG], PATTERN, max_hits=max_hits)
    assert found.count == len(HITS) and found.positions.tolist() == list(HITS[:k]) and found.size == LONG


# ---------------------------------------------------------------- planes and records
def test_planes_of_single_bytes(long, shafa):
    """E = 1 and 2^32 + delta elements: both sides cross the boundary and the transpose is the identity"""
    import torch
    long.random_a(4)
    long.b.fill_(FILL)
    call(shafa, 1, lambda bt, st: bt.split_planes_dev(st, 1, long.a, [LEAD], [LONG], i64([LONG]), long.b, [LEAD]))
    assert torch.equal(long.b[LEAD:LEAD + LONG], long.a[LEAD:LEAD + LONG])
    assert untouched(long.b, LEAD, LEAD + LONG)
    out = long.third()
    call(shafa, 1, lambda bt, st: bt.merge_planes_dev(st, 1, long.b, [LEAD], [LONG], i64([LONG]), out, [LEAD + 5]))
    assert torch.equal(out[LEAD + 5:LEAD + 5 + LONG], long.a[LEAD:LEAD + LONG])
    assert untouched(out, LEAD + 5, LEAD + 5 + LONG)


def _columns(long, shafa, w, n, split, merge):
    """n records of w bytes in a, their columns al16(n) apart in b, and back at an odd offset of a third allocation"""
    import torch
    long.random_a(5 + w, n * w)
    long.b.fill_(FILL)
    pitch = al16(n)
    poff = [LEAD + j * pitch for j in range(w)]
    assert n * w > G and poff[-1] + pitch <= ALLOC - GUARD
    call(shafa, 1, lambda bt, st: getattr(bt, split)(st, w, long.a, [LEAD], [n], i64([n]), long.b, poff))
    cols = long.b.as_strided((w, n), (pitch, 1), LEAD)
    assert torch.equal(cols, torch_planes(long.a[LEAD:LEAD + n * w], w))
    assert bool((long.b.as_strided((w, pitch - n), (pitch, 1), LEAD + n) == FILL).all()) and untouched(long.b, LEAD, LEAD + w * pitch)
    out = long.third()
    call(shafa, 1, lambda bt, st: getattr(bt, merge)(st, w, long.b, poff, [n], i64([n]), out, [LEAD + 5]))
    assert torch.equal(out[LEAD + 5:LEAD + 5 + n * w], long.a[LEAD:LEAD + n * w])
    assert untouched(out, LEAD + 5, LEAD + 5 + n * w)


def test_planes_of_four_bytes(long, shafa):
    _columns(long, shafa, 4, (1 << 30) + DELTA, "split_planes_dev", "merge_planes_dev")


def test_records_of_three_bytes(long, shafa):
    _columns(long, shafa, 3, G // 3 + DELTA, "split_records_dev", "merge_records_dev")


# ---------------------------------------------------------------- Lorenzo differences
def test_grid_planes_and_histograms(long, shafa):
    """E = 4, lags 1, 4099 and 2^29 + 3 elements: the last tap of an element behind byte 2^32 lies 2 GiB in front of it"""
    import torch
    n, k = (1 << 30) + DELTA, 4
    lags = (1, 4099, (1 << 29) + 3)
    long.random_a(9, n * k)
    long.b.fill_(FILL)
    pitch = al16(n)
    poff = [LEAD + j * pitch for j in range(k)]
    d_n = i64([n])
    d_freq = torch.full((k * 256,), -1, dtype=torch.int64, device=DEV)
    call(shafa, 1, lambda bt, st: bt.split_planes_grid_dev(st, k, [lags], long.a, [LEAD], [n], d_n, long.b, poff))
    call(shafa, 1, lambda bt, st: bt.hist_planes_grid_dev(st, k, [lags], long.a, [LEAD], [n], d_n, d_freq))
    z = torch_grid_z(long.a[LEAD:LEAD + n * k].view(torch.int32), lags)
    assert torch.equal(long.b.as_strided((k, n), (pitch, 1), LEAD), torch_planes(z.view(torch.uint8), k))
    assert untouched(long.b, LEAD, LEAD + k * pitch)
    assert torch.equal(d_freq.view(k, 256), torch_plane_hist(z))
    del z
    torch.cuda.empty_cache()
    out = long.third()
    call(shafa, 1, lambda bt, st: bt.merge_planes_grid_dev(st, k, [lags], long.b, poff, [n], d_n, out, [LEAD + 4]))
    assert torch.equal(out[LEAD + 4:LEAD + 4 + n * k], long.a[LEAD:LEAD + n * k])
    assert untouched(out, LEAD + 4, LEAD + 4 + n * k)


# ---------------------------------------------------------------- a .shaf file past 4 GiB
BIG, NBIG = 64 << 20, 64
SPAN = 1024


def shaf_layout(sizes):
    """(the frame texts, where each payload starts, the file's length) of a .shaf of payloads of these sizes: "@n", then
    "@size@" and the payload per block"""
    texts, places, pos = [], [], 0
    for b, n in enumerate(sizes):
        t = (b"@" + str(len(sizes)).encode() if b == 0 else b"") + b"@" + str(n).encode() + b"@"
        texts.append(t)
        pos += len(t)
        places.append(pos)
        pos += n
    return texts, places, pos


def real_blocks(oracle):
    """two blocks under one 12-bit table with the oracle's streams, the first cut so that, behind a payload at a multiple of 16,
    the second one's payload starts at a multiple of 16 too: the decoders take their input at such offsets"""
    from test_gpu_parity import long_code_case
    tab, one = long_code_case(oracle, 70000, 13, 0.5, 8)
    _, two = long_code_case(oracle, 40001, 13, 0.5, 9)
    rc, s2 = oracle.sf_encode(two, tab)
    assert rc == 0
    for n in range(65613, 65613 + 400):
        rc, s1 = oracle.sf_encode(np.ascontiguousarray(one[:n]), tab)
        assert rc == 0
        if (s1.size + len(b"@%d@" % s2.size)) % 16 == 0:
            return tab, [np.ascontiguousarray(one[:n]), two], [s1, s2]
    raise AssertionError("no cut of the first block aligns the second")


def test_shaf_file_past_4_gib(long, shafa, oracle):
    """64 payloads of 64 MiB from a window sliding over 128 MiB of random bytes, then two real blocks, whose payloads lie past
    byte 2^32 of the file: pack_payloads, unpack_shaf, unpack_payloads, sf_decode_dev, seek_index_dev and read_spans_dev"""
    import torch
    from test_gpu_far_offsets import table_bytes
    tab, plain, streams = real_blocks(oracle)
    nb = NBIG + 2
    sizes = [BIG] * NBIG + [s.size for s in streams]
    sizes[NBIG - 1] -= (shaf_layout(sizes)[1][NBIG]) % 16                   # the first real payload at a multiple of 16
    texts, places, total = shaf_layout(sizes)
    assert places[NBIG] % 16 == 0 and places[NBIG + 1] % 16 == 0 and places[NBIG] > G and total <= ALLOC - LEAD - GUARD
    src = torch.empty((128 << 20) + al16(streams[0].size) + al16(streams[1].size), dtype=torch.uint8, device=DEV)
    src[:128 << 20] = random_period(11, 128 << 20, DEV)
    src_off = [b << 20 for b in range(NBIG)] + [128 << 20, (128 << 20) + al16(streams[0].size)]
    for o, s in zip(src_off[NBIG:], streams):
        src[o:o + s.size] = torch.from_numpy(s).to(DEV)
    long.a.fill_(FILL)
    long.b.fill_(FILL)
    file = long.a[LEAD:LEAD + total]
    d_len = i64([-1])
    call(shafa, nb, lambda bt, st: bt.pack_payloads(st, shafa.FRAME_SHAF, src, src_off, sizes, i64(sizes), long.a[LEAD:], total, d_len))
    assert int(d_len[0]) == total and untouched(long.a, LEAD, LEAD + total)
    for b in range(nb):
        t = texts[b]
        assert bytes(file[places[b] - len(t):places[b]].cpu().numpy()) == t, f"frame text of block {b}"
        assert torch.equal(file[places[b]:places[b] + sizes[b]], src[src_off[b]:src_off[b] + sizes[b]]), f"payload {b}"
    # the parse
    d_count = torch.zeros(8, dtype=torch.int64, device=DEV)
    d_count[0] = nb
    d_off, d_n = i64([-1] * nb), i64([-1] * nb)
    call(shafa, nb, lambda bt, st: bt.unpack_shaf(st, nb, file, d_count, d_off, d_n))
    assert d_off.tolist() == places and d_n.tolist() == sizes
    # the last four payloads to 16-aligned regions of b
    last = range(nb - 4, nb)
    dst, pos = [], LEAD
    for b in last:
        dst.append(pos)
        pos += al16(sizes[b]) + GUARD
    call(shafa, 4, lambda bt, st: bt.unpack_payloads(st, file, d_off[nb - 4:], d_n[nb - 4:], long.b, dst, [al16(sizes[b]) for b in last]))
    for o, b in zip(dst, last):
        assert torch.equal(long.b[o:o + sizes[b]], src[src_off[b]:src_off[b] + sizes[b]]), f"unpacked payload {b}"
    assert untouched(long.b, LEAD, pos - GUARD)
    # the two real blocks decoded from where they lie in the file
    long.b.fill_(FILL)
    _, d_tables = table_bytes(shafa, [tab, tab])
    nsym = [p.size for p in plain]
    out = [LEAD + G, LEAD + G + al16(nsym[0]) + GUARD]
    pay = [LEAD + places[NBIG], LEAD + places[NBIG + 1]]
    call(shafa, 2, lambda bt, st: bt.sf_decode_dev(st, long.a, pay, sizes[NBIG:], i64(sizes[NBIG:]), d_tables, i64(nsym), long.b, out, nsym))
    for o, p in zip(out, plain):
        assert bytes(long.b[o:o + p.size].cpu().numpy()) == p.tobytes()
    assert untouched(long.b, out[0], out[1] + al16(nsym[1]))
    # their seek index from the decoded bytes, and ranges read back from the file through it
    first, ckpt = [], []
    for p in plain:
        first.append(len(ckpt) // 2)
        bits = np.concatenate([[0], np.cumsum(tab.lens()[p].astype(np.int64))])
        for k in range(-(-p.size // SPAN)):
            ckpt += [int(bits[k * SPAN]), k * SPAN]
    d_ckpt, d_status, d_dec = i64([-1] * len(ckpt)), torch.full((2,), -1, dtype=torch.int32, device=DEV), i64([-1, -1])
    call(shafa, 2, lambda bt, st: bt.seek_index_dev(st, long.b, out, nsym, i64(nsym), d_tables, SPAN, shafa.SEEK_SF, first, d_ckpt,
                                                    d_status, d_dec))
    assert d_ckpt.tolist() == ckpt and d_status.tolist() == [0, 0] and d_dec.tolist() == nsym
    ranges = [(0, 0, nsym[0]), (1, SPAN // 2 + 1, nsym[1] - SPAN - 7)]
    back = [LEAD + G - (1 << 20), LEAD + G + (1 << 19) + 5]
    assert back[0] + nsym[0] + GUARD <= out[0] and out[1] + nsym[1] + 2 * GUARD <= back[1] and back[1] + nsym[1] + GUARD <= ALLOC
    items = [(b, lo // SPAN, (hi - 1) // SPAN, lo, hi, o) for (b, lo, hi), o in zip(ranges, back)]
    call(shafa, 2, lambda bt, st: bt.read_spans_dev(st, file, places[NBIG:], sizes[NBIG:], nsym, first, d_tables, SPAN, shafa.SEEK_SF,
                                                    d_ckpt, items, long.b))
    for (b, lo, hi), o in zip(ranges, back):
        assert bytes(long.b[o:o + hi - lo].cpu().numpy()) == plain[b][lo:hi].tobytes(), (b, lo, hi)
        assert untouched(long.b, o, o + hi - lo)


def test_peak_memory(long):
    import torch
    peak = torch.cuda.max_memory_allocated()
    print("peak device memory of the long regions:", peak)
    assert peak <= LIMIT
