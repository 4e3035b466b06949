"""Unsynchronised launch sequences on ONE batch (csrc/api.hip: the staging ring, the two parameter buffers, batch_upload, the
shared workspace, the error words, the change of stream), every launch of a sequence against the oracle.

The library is used as its header says: calls "enqueue work on `stream` and return without synchronising".  The other GPU
tests run one launch (or one dependent chain) per finish on a fresh batch; here a `Sequence` of many independent launches of
the layer-2 entry points is enqueued on one batch and finished ONCE.  Every launch owns its input regions, its 16-byte
aligned output regions in one output tensor filled with 0xEE (at least 48 guard bytes behind every block) and its
d_out_n / d_freq / d_crc slots; everything it needs lies in device memory BEFORE the first enqueue, and between the first
enqueue and the single finish the tests call nothing that synchronises (no .cpu(), no allocation, no fill_) — except where a
case says so: the batch's own growth in case 1 and the stream change in case 7.

What a launch must leave comes from the CPU alone and does not depend on its place in the sequence:
    hist256                       oracle.hist256
    rle_encode (with, without d_freq)   oracle.rle_encode, oracle.hist256 of it
    sf_encode                     oracle.sf_build, oracle.sf_encode
    sf_decode                     oracle.sf_decode of the oracle's stream (asserted equal to the data)
    rle_decode                    oracle.rle_decode of the oracle's .rle bytes
    sf_build_codes                the host's Module T (shafa.sf_build_codes_batch)
    sf_encode_dev, sf_decode_dev  the oracle's stream / the data, fed by tables in device memory
    crc32_dev                     zlib.crc32
Launches pick different members of a pool of (data, table) pairs in different orders, so that no two launches of a sequence
share tables, sizes and output offsets: a launch that ran with another launch's records leaves its own regions 0xEE or wrong.

Measured on an MI355X: see LABNOTES.md, "Launch sequences"."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_gpu_parity import first_diff, to_shafa_table

gpu = pytest.mark.gpu             # every test but the CPU test of the shapes

FILL = 0xEE
GUARD = 48                        # bytes behind every block's output region that nobody may write
FRONT = 64                        # bytes in front of the first block
SENT = 0x6E6E6E6E6E6E6E6E         # what the size / count slots hold before a launch writes them
SENT32 = 0x6E6E6E6E
KIB, MIB = 1024, 1 << 20

FILE_UNRECOGNIZABLE, LACK_OF_MEMORY = 4, 2          # include/shafa_hip.h, enum shafa_error (asserted against the package)


def al16(x):
    return (x + 15) // 16 * 16


# ---------------------------------------------------------------- the pool
class Item:
    """one (data, table) pair and what the CPU says every entry point makes of it (computed when first asked for)"""

    def __init__(self, oracle, name, data, tfreq=None):
        self.o, self.name = oracle, name
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.n = int(self.data.size)
        self.hist = oracle.hist256(self.data)
        self.tfreq = self.hist if tfreq is None else np.ascontiguousarray(tfreq, dtype=np.uint64)   # what Module T is given
        self.tab = oracle.sf_build(self.tfreq)
        self.lens = self.tab.lens()
        self.lmax = int(self.lens.max())
        self.tab_bytes = bytes(self.tab)
        self._enc = self._rle = self._rle_hist = self._stab = self._npre = None
        self.crc = zlib.crc32(self.data.tobytes())

    @property
    def enc(self):
        if self._enc is None:
            rc, e = self.o.sf_encode(self.data, self.tab)
            assert rc == 0
            rc, back = self.o.sf_decode(e, self.tab, self.n)          # the decoders' reference: the oracle's own decode
            assert rc == 0 and back.tobytes() == self.data.tobytes()
            self._enc = e
        return self._enc

    @property
    def rle(self):
        if self._rle is None:
            r = self.o.rle_encode(self.data)
            rc, back = self.o.rle_decode(r, cap=self.n)
            assert rc == 0 and back.tobytes() == self.data.tobytes()
            self._rle, self._rle_hist = r, self.o.hist256(r)
        return self._rle

    @property
    def rle_hist(self):
        self.rle
        return self._rle_hist

    def stab(self, shafa):
        if self._stab is None:
            self._stab = to_shafa_table(shafa, self.tab)
        return self._stab

    def n_prefixes(self):
        """distinct proper prefixes of the codes, the empty one included: the inner nodes of the code's trie"""
        if self._npre is None:
            seen = {""}
            for s in np.nonzero(self.lens)[0]:
                c = self.tab.code_str(int(s))
                seen.update(c[:k] for k in range(1, len(c)))
            self._npre = len(seen)
        return self._npre


def _long_code_item(oracle, n, seed):
    """a table with a longest code of 14 .. 16 bits (counts that halve: test_gpu_parity.long_code_case's histogram) and data
    that uses every one of its symbols"""
    nsyms = 17
    freq = np.zeros(256, dtype=np.uint64)
    for i in range(nsyms):
        freq[(i * 7) % 256] = max(1, int(2.0 ** 50 * 0.5 ** i))
    syms = np.array([(i * 7) % 256 for i in range(nsyms)], dtype=np.uint8)
    r = oracle.gen_bytes(seed, n).astype(np.int64)
    data = syms[np.minimum((r * r * nsyms) // (255 * 255 + 1), nsyms - 1)]
    data[:nsyms] = syms
    it = Item(oracle, f"long16/{n}", data, tfreq=freq)
    assert 14 <= it.lmax <= 16, it.lmax
    return it


_zipf = None


def _make(oracle, kind, n, seed):
    import golden.make_golden as mg
    global _zipf
    if _zipf is None:
        _zipf = mg.zipf_mod256_table(1.2)
    zt = _zipf
    if kind == "zipf":
        data = oracle.gen_bytes(seed, n, zt)
    elif kind == "runs":
        data = mg.runs_stream(seed, n, zt)
    elif kind == "uniform":
        data = oracle.gen_bytes(seed, n)
    elif kind == "two":
        data = (oracle.gen_bytes(seed, n) & 1).astype(np.uint8) * 200 + 3
    else:
        return _long_code_item(oracle, n, seed)
    return Item(oracle, f"{kind}/{n}", data)


class Pool:
    """24 pairs of 600 B .. 70 KiB (Zipf(1.2) mod 256, runs streams, uniform bytes, two-symbol blocks, one table with a
    14 .. 16-bit longest code), two blocks of about 1.5 MiB for the growth case, and 48 blocks of 8 .. 40 KiB with 48
    different tables for the launches that fill the staging ring"""
    SMALL = [("zipf", 600), ("runs", 611), ("uniform", 640), ("zipf", 655), ("two", 673), ("runs", 689), ("uniform", 700),
             ("zipf", 617)]
    MID = [("zipf", 8197), ("runs", 9001), ("uniform", 12289), ("zipf", 16384), ("runs", 16401), ("long16", 20011),
           ("two", 24577), ("zipf", 28001), ("runs", 32768), ("uniform", 33333), ("zipf", 36865), ("runs", 40950)]
    LARGE = [("zipf", 45001), ("runs", 57351), ("uniform", 65536), ("zipf", 70001)]
    BIG = [("zipf", 3 * MIB // 2 + 77), ("runs", 3 * MIB // 2 - 4099)]

    def __init__(self, oracle):
        self.o = oracle
        mk = lambda spec, seed0: [_make(oracle, k, n, seed0 + i) for i, (k, n) in enumerate(spec)]
        self.small, self.mid, self.large = mk(self.SMALL, 1100), mk(self.MID, 1200), mk(self.LARGE, 1300)
        self.big = mk(self.BIG, 1400)
        self.all24 = self.small + self.mid + self.large
        assert all(600 <= it.n <= 70 * KIB for it in self.all24)
        assert len({it.tab_bytes for it in self.all24}) == len(self.all24), "two pool members share a table"
        assert len({it.n for it in self.all24 + self.big}) == len(self.all24) + 2
        self._t48 = None

    @property
    def t48(self):
        if self._t48 is None:
            self._t48 = [_make(self.o, ("zipf", "runs", "zipf")[i % 3], 8192 + 683 * i + (i % 7), 2000 + i) for i in range(48)]
            assert all(8 * KIB <= it.n <= 40 * KIB for it in self._t48)
            assert len({it.tab_bytes for it in self._t48}) == 48, "the 48 tables are not all different"
        return self._t48


_pool = None


@pytest.fixture(scope="module")
def pool(oracle):
    global _pool
    if _pool is None:
        _pool = Pool(oracle)
    return _pool


def pick(group, count, k):
    """`count` members of `group` in an order that depends on k (whole permutations of the group, one after the other):
    launches with different k walk the group differently"""
    rng = np.random.default_rng(7000 + k)
    order = np.concatenate([rng.permutation(len(group)) for _ in range(-(-count // len(group)))])
    return [group[j] for j in order[:count]]


# ---------------------------------------------------------------- the plans (pure Python: the CPU test reads them too)
# A plan is a list of (kind, items, options).  Kinds: hist, rle_enc (option freq), sf_enc, sf_dec, rle_dec, crc, build
# (sf_build_codes), sf_enc_dev (option tables_from = index of the build launch whose tables it takes, else uploaded tables),
# sf_dec_dev.  "tc" below stands for build + sf_enc_dev on the same blocks.
ROUND_KINDS = ("hist", "rle_enc_f", "rle_enc", "sf_enc", "sf_dec", "rle_dec", "tc", "sf_dec_dev", "crc")


def add(plan, kind, items, **opts):
    if kind == "tc":
        plan.append(("build", items, {}))
        plan.append(("sf_enc_dev", items, dict(opts, tables_from=len(plan) - 1)))
    elif kind == "rle_enc_f":
        plan.append(("rle_enc", items, dict(opts, freq=True)))
    else:
        plan.append((kind, items, opts))


def plan_round(plan, group, count, k0):
    for i, kind in enumerate(ROUND_KINDS):
        add(plan, kind, pick(group, count, k0 + i))


def plan_growing(pool):
    """case 1 and 2: a round of every entry point on 3 blocks, on 40 blocks of 8 .. 70 KiB, on the two 1.5 MiB blocks, then
    sf_encode and sf_decode on 512 blocks of about 600 B.  Returns the plan and the number of launches of the first round."""
    plan = []
    plan_round(plan, pool.all24, 3, 0)
    first = len(plan)
    plan_round(plan, pool.mid + pool.large, 40, 20)
    for i, kind in enumerate(ROUND_KINDS):
        add(plan, kind, pool.big if i % 2 else pool.big[::-1])
    add(plan, "sf_enc", pick(pool.small, 512, 40))
    add(plan, "sf_dec", pick(pool.small, 512, 41))
    return plan, first


ENTRIES = ("hist", "rle_enc", "sf_enc", "sf_dec", "rle_dec", "crc", "tc", "sf_dec_dev")


def every_pair_order(nodes):
    """a walk through the complete directed graph on `nodes`, loops included, that takes every edge once (Hierholzer):
    len(nodes)^2 + 1 entries in which every ordered pair is adjacent"""
    out_edges = {a: list(nodes[::-1]) for a in nodes}
    stack, walk = [nodes[0]], []
    while stack:
        a = stack[-1]
        if out_edges[a]:
            stack.append(out_edges[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def plan_pairs(pool):
    """case 3: one rle_encode of a 1.5 MiB block (a large, dirty workspace), then every entry point right after every other"""
    plan = []
    add(plan, "rle_enc", [pool.big[0]])
    group = pool.small + pool.mid[:4]
    for k, e in enumerate(every_pair_order(ENTRIES)):
        add(plan, "rle_enc_f" if e == "rle_enc" and k % 2 else e, pick(group, 3 + k % 4, k))
    return plan


def entries_of(plan):
    """the plan as a list of entry points, build + sf_enc_dev on the same blocks counted as one"""
    out = []
    for kind, _, opts in plan:
        if kind == "sf_enc_dev" and "tables_from" in opts:
            assert out[-1] == "build"
            out[-1] = "tc"
        else:
            out.append(kind)
    return out


RING_PAIRS = 16


def plan_ring(pool):
    """case 4: sf_encode of 512 blocks of about 600 B and sf_decode of 48 blocks of 8 .. 40 KiB with 48 different tables, in
    turn, every launch with another permutation"""
    plan = []
    for k in range(RING_PAIRS):
        add(plan, "sf_enc", pick(pool.small, 512, 2 * k))
        add(plan, "sf_dec", pick(pool.t48, 48, 2 * k + 1))
    return plan


PARAM_ORDER = "SLSSLLSLLLSSSL"
S_KINDS = ("sf_dec", "sf_enc_dev", "sf_enc", "sf_dec_dev")      # 2 blocks: below PARAMS_INLINE_BYTES
L_KINDS = ("sf_enc", "sf_dec")     # 64 blocks; the _dev entries stage 48 / 40 bytes a block and cannot pass 64 KiB with 64


def plan_params(pool):
    """case 5: the two parameter buffers take inline (S) and side-stream (L) uploads in the order PARAM_ORDER, then
    rle_encode / rle_decode of 600 blocks (batch_upload's kernel) between launches of 3 blocks (its hipMemcpyAsync).
    Returns the plan and the letters of its first launches."""
    plan, ns, nl = [], 0, 0
    for k, c in enumerate(PARAM_ORDER):
        if c == "S":
            add(plan, S_KINDS[ns % 4], pick(pool.small, 2, k))
            ns += 1
        else:
            add(plan, L_KINDS[nl % 2], pick(pool.mid, 64, k))
            nl += 1
    add(plan, "rle_enc_f", pick(pool.small, 3, 50))
    add(plan, "rle_enc_f", pick(pool.small, 600, 51))
    add(plan, "rle_dec", pick(pool.small, 600, 52))
    add(plan, "rle_dec", pick(pool.small, 3, 53))
    return plan


# ---------------------------------------------------------------- what the launchers stage (mirrored from csrc)
RING_FACTOR, RING_EXTRA = 4, 1 << 20          # api.hip:87        const size_t want = 4 * bytes + (1 << 20);
STAGE_UNIT = 64                               # api.hip:73        bytes = (bytes + 63) & ~(size_t)63;
PARAMS_INLINE_BYTES = 64 * 1024               # internal.hpp:20   constexpr size_t PARAMS_INLINE_BYTES = 64 * 1024;
UPLOAD_KERNEL_ABOVE = 16384                   # api.hip:152       if (b->par_dma || bytes <= 16384 || ...) hipMemcpyAsync
ENC_BLK = 80                                  # internal.hpp:106  struct EncBlk: 7 pointers / u64, 4 u32, 1 pointer
ENC_TAB_MIN, ENC_TAB_MAX = 1024, 2048         # sf_encode.hip:300 tab1 = one_pass ? 2048 : 1024; :314 class 2: 2048
DEC_BLK = 184                                 # sfd_common.hpp:30 struct DecBlk: 19 pointers / u64, 8 u32
LUT_MAXK, LEN_MAXK, SYM3_MAXK = 11, 13, 12    # sfd_common.hpp:14, :28, :22
LUT2_MAX = 4096                               # sfd_common.hpp:15
LONG_BYTES = 16 + 128 * 2 + 128 * 16 * 2      # sfd_common.hpp:25
LONG32_BYTES = 16 + 128 * 2 + 128 * 2 + 256 * 4 + 128 * 2      # sfd_common.hpp:27
PLAN_BLK, SDV_HOST = 48, 40                   # sf_encode_dev.hip:41, :185 / sfd_dev.hpp:30, :380: all that the _dev entries stage
RLE_BLK, RLD_BLK = 72, 64                     # rle_encode.hip:28, :1069 / rle_decode.hip:47, :466


def dec_table_bounds(it):
    """bytes of look-up tables sfdec_launch stages for one running block (sf_decode.hip:1545-1548), from below and from above.
    Sizes: sfd_host_tables.hpp:27-31 (lut: 2^K u16, lenlut: 2^K1 + 4 u8, lut13: 2^K1 + 2 u16), :19-52 (trie: a pair of u32
    per inner node), :78-84 (long32, when a code has more than SYM3_MAXK bits), :130-131 (lenlut32, more than LEN_MAXK),
    :152 (longtab, at most 16 bits and more than SYM3_MAXK), :184-196 (lut2: at most LUT2_MAX entries and one of padding)"""
    K, K1 = min(it.lmax, LUT_MAXK), min(it.lmax, LEN_MAXK)
    lut, lenlut, lut13, trie = 2 << K, (1 << K1) + 4, 2 * ((1 << K1) + 2), 8 * it.n_prefixes()
    lo = lut + lenlut + lut13 + trie + 16
    hi = lut + lenlut + lut13 + trie + 16 + 5 * 15
    if it.lmax > LUT_MAXK:
        hi += 2 * (LUT2_MAX + 1)
    if it.lmax > SYM3_MAXK:
        hi += LONG_BYTES + LONG32_BYTES + 15
    if it.lmax > LEN_MAXK:
        hi += lenlut + 15
    return lo, hi


def staged_bounds(kind, items):
    """(lower, upper) bound of the bytes a launch asks the staging ring for; for sf_enc / sf_dec / the _dev entries these are
    its parameter bytes (batch_params_begin), for the others what batch_upload copies"""
    nb = len(items)
    if kind == "sf_enc":                           # sf_encode.hip:310-315, :321: EncBlk array, 16-byte aligned, + tables
        assert all(1 <= it.lmax <= 32 and it.n for it in items)        # classes 1 and 2: every block runs
        return nb * (ENC_BLK + ENC_TAB_MIN), al16(nb * ENC_BLK) + nb * ENC_TAB_MAX
    if kind == "sf_dec":                           # sf_decode.hip:1571-1574: DecBlk array, run_dp words, tables
        assert all(it.lmax >= 1 and it.n for it in items)
        b = [dec_table_bounds(it) for it in items]
        return nb * DEC_BLK + sum(x[0] for x in b), al16(nb * DEC_BLK) + al16(nb * 4) + sum(x[1] for x in b)
    if kind == "sf_enc_dev":
        return nb * PLAN_BLK, nb * PLAN_BLK
    if kind == "sf_dec_dev":
        return nb * SDV_HOST, nb * SDV_HOST
    if kind == "rle_enc":
        return nb * RLE_BLK, nb * RLE_BLK
    if kind == "rle_dec":
        return nb * RLD_BLK, nb * RLD_BLK
    raise AssertionError(kind)


def test_sequence_shapes(pool):
    """CPU only: the plans have the shapes the GPU cases are named after.
    (3) every ordered pair of entry points is adjacent; (4) the launches of the ring case ask for more than twice the
    largest ring there can be, so it wraps whatever the exact record sizes are; (5) the S and L launches lie on the sides of
    PARAMS_INLINE_BYTES, and the RLE launches of 600 and of 3 blocks on the sides of batch_upload's 16 KiB."""
    e = entries_of(plan_pairs(pool))
    have = set(zip(e, e[1:]))
    missing = [(a, b) for a in ENTRIES for b in ENTRIES if (a, b) not in have]
    assert not missing, missing
    assert all(3 <= len(items) <= 6 for _, items, _ in plan_pairs(pool)[1:])

    ring = plan_ring(pool)
    assert len(ring) >= 24
    bounds = [staged_bounds(kind, items) for kind, items, _ in ring]
    ring_max = RING_FACTOR * (max(hi for _, hi in bounds) + STAGE_UNIT) + RING_EXTRA
    asked = sum(lo for lo, _ in bounds)
    assert asked > 2 * ring_max, (asked, ring_max)

    par = plan_params(pool)
    for c, (kind, items, _) in zip(PARAM_ORDER, par):
        lo, hi = staged_bounds(kind, items)
        assert (hi <= PARAMS_INLINE_BYTES) if c == "S" else (lo > PARAMS_INLINE_BYTES), (c, kind, len(items), lo, hi)
    sides = [staged_bounds(kind, items) for kind, items, _ in par[len(PARAM_ORDER):]]
    assert [len(items) for _, items, _ in par[len(PARAM_ORDER):]] == [3, 600, 600, 3]
    assert sides[0][1] <= UPLOAD_KERNEL_ABOVE < sides[1][0] and sides[2][0] > UPLOAD_KERNEL_ABOVE >= sides[3][1]
    keys = [(kind, tuple(id(it) for it in items)) for kind, items, _ in par]
    assert len(set(keys)) == len(keys), "two launches of the parameter case are the same"

    grow, first = plan_growing(pool)
    assert sum(lo_hi[1] for lo_hi in (staged_bounds(k, i) for k, i, _ in grow[:first]
                                      if k in ("sf_enc", "sf_dec", "sf_enc_dev", "sf_dec_dev", "rle_enc", "rle_dec"))) < MIB


# ---------------------------------------------------------------- the harness
class Launch:
    pass


class Sequence:
    """the launches of a plan with their regions in the shared tensors; prepare() uploads everything, enqueue() only calls
    the entry points, check() reads everything back once and returns the list of problems"""

    def __init__(self, shafa, oracle, plan, name=""):
        self.shafa, self.o, self.name = shafa, oracle, name
        self.tsz = C.sizeof(shafa.CodeTable)
        self.L = []
        for idx, (kind, items, opts) in enumerate(plan):
            L = Launch()
            L.idx, L.kind, L.items, L.opts, L.nb = idx, kind, list(items), dict(opts), len(items)
            self.L.append(L)

    # -- per block: input bytes, expected output bytes, output capacity
    def _block(self, L, i):
        it, k = L.items[i], L.kind
        if k in ("hist", "crc", "rle_enc", "sf_enc", "sf_enc_dev"):
            src = it.data
        elif k in ("sf_dec", "sf_dec_dev"):
            src = it.enc
            if i in L.opts.get("cut", ()):
                src = src[:src.size // 2]
        elif k == "rle_dec":
            src = it.rle
        else:
            src = None
        if k == "rle_enc":
            want, cap = it.rle, it.rle.size                    # exact room: the header's rule for rle_encoded_size_dev's sizes
        elif k in ("sf_enc", "sf_enc_dev"):
            want, cap = it.enc, al16(it.enc.size) + 16
            if i in L.opts.get("small_cap", ()):
                cap = (it.enc.size // 2) // 16 * 16
        elif k in ("sf_dec", "sf_dec_dev", "rle_dec"):
            want, cap = it.data, it.n
        else:
            want, cap = None, 0
        return src, want, cap

    def prepare(self):
        import torch
        sh = self.shafa
        dev = torch.device("cuda", 0)
        ipos, opos, npos, fpos, cpos, spos, tipos, topos, fipos = 0, FRONT, 0, 0, 0, 0, 0, 0, 0
        ins, self.regions = [], []                              # regions: (launch, block, off, cap) in the order of the offsets
        for L in self.L:
            L.in_off, L.in_n, L.in_cap, L.out_off, L.out_cap, L.want = [], [], [], [], [], []
            for i in range(L.nb):
                src, want, cap = self._block(L, i)
                if src is not None:
                    L.in_off.append(ipos)
                    L.in_n.append(int(src.size))
                    L.in_cap.append(al16(src.size))
                    ins.append((ipos, src))
                    ipos += al16(src.size) + 16
                if want is not None:
                    L.out_off.append(opos)
                    L.out_cap.append(cap)
                    L.want.append(want)
                    self.regions.append((L, i, opos, cap))
                    opos += al16(cap) + GUARD
            k = L.kind
            if k in ("rle_enc", "sf_enc", "sf_enc_dev", "rle_dec"):
                L.n0, npos = npos, npos + L.nb + 1
            if k == "hist" or (k == "rle_enc" and L.opts.get("freq")):
                L.f0, fpos = fpos, fpos + L.nb * 256 + 8
            if k == "crc":
                L.c0, cpos = cpos, cpos + L.nb + 1
            if k in ("crc", "sf_enc_dev", "sf_dec_dev"):
                L.s0, spos = spos, spos + 2 * L.nb
            if k == "sf_dec_dev" or (k == "sf_enc_dev" and "tables_from" not in L.opts):
                L.ti0, tipos = tipos, tipos + L.nb
            if k == "build":
                L.to0, topos = topos, topos + L.nb + 1
                L.fi0, fipos = fipos, fipos + L.nb * 256
        h_in = np.zeros(ipos + 64, dtype=np.uint8)
        for o, src in ins:
            h_in[o:o + src.size] = src
        h_sz = np.zeros(spos + 1, dtype=np.int64)
        h_ti = np.zeros((tipos + 1) * self.tsz, dtype=np.uint8)
        h_fi = np.zeros(fipos + 1, dtype=np.uint64)
        for L in self.L:
            k = L.kind
            if k in ("crc", "sf_enc_dev", "sf_dec_dev"):
                h_sz[L.s0:L.s0 + L.nb] = L.in_n
                h_sz[L.s0 + L.nb:L.s0 + 2 * L.nb] = [it.n for it in L.items]
            if hasattr(L, "ti0"):
                for i, it in enumerate(L.items):
                    h_ti[(L.ti0 + i) * self.tsz:(L.ti0 + i + 1) * self.tsz] = np.frombuffer(it.tab_bytes, dtype=np.uint8)
            if k == "build":
                for i, it in enumerate(L.items):
                    h_fi[L.fi0 + i * 256:L.fi0 + (i + 1) * 256] = it.tfreq
                host = sh.sf_build_codes_batch(np.stack([it.tfreq for it in L.items]))       # the host's Module T
                L.want_tabs = [bytes(host[i]) for i in range(L.nb)]
                for i, it in enumerate(L.items):           # the encoder behind it is compared with the ORACLE's stream of the
                    assert L.want_tabs[i] == it.tab_bytes  # oracle's table: the two Module Ts agree on these counts
            if k in ("sf_enc", "sf_dec"):
                tabs = [it.stab(sh) for it in L.items]
                for i in L.opts.get("bad_table", ()):
                    tabs[i] = self._not_prefix_free(L.items[i])
                L.tarr = sh.Batch._tables(tabs)
        self.opos, self.npos, self.fpos, self.cpos, self.topos = opos, npos, fpos, cpos, topos
        self.d_in = torch.from_numpy(h_in).to(dev)
        self.d_sz = torch.from_numpy(h_sz).to(dev)
        self.d_ti = torch.from_numpy(h_ti).to(dev)
        self.d_fi = torch.from_numpy(h_fi.view(np.int64)).to(dev)
        self.d_out = torch.empty(opos + 64, dtype=torch.uint8, device=dev)
        self.d_n = torch.empty(npos + 1, dtype=torch.int64, device=dev)
        self.d_freq = torch.empty(fpos + 1, dtype=torch.int64, device=dev)
        self.d_crc = torch.empty(cpos + 1, dtype=torch.int32, device=dev)
        self.d_to = torch.empty((topos + 1) * self.tsz, dtype=torch.uint8, device=dev)
        for L in self.L:                                   # the calls' arguments: views made now, nothing is made later
            k, s = L.kind, None
            if hasattr(L, "s0"):
                s = (self.d_sz[L.s0:L.s0 + L.nb], self.d_sz[L.s0 + L.nb:L.s0 + 2 * L.nb])
            if k == "hist":
                L.call = ("hist256", (self.d_in, L.in_off, L.in_n, self.d_freq[L.f0:]))
            elif k == "rle_enc":
                L.call = ("rle_encode", (self.d_in, L.in_off, L.in_n, self.d_out, L.out_off, L.out_cap, self.d_n[L.n0:],
                                         self.d_freq[L.f0:] if hasattr(L, "f0") else None))
            elif k == "sf_enc":
                L.call = ("sf_encode", (self.d_in, L.in_off, L.in_n, L.tarr, self.d_out, L.out_off, L.out_cap, self.d_n[L.n0:]))
            elif k == "sf_dec":
                L.call = ("sf_decode", (self.d_in, L.in_off, L.in_n, L.tarr, [it.n for it in L.items], self.d_out, L.out_off))
            elif k == "rle_dec":
                L.call = ("rle_decode", (self.d_in, L.in_off, L.in_n, self.d_out, L.out_off, L.out_cap, self.d_n[L.n0:]))
            elif k == "crc":
                L.call = ("crc32_dev", (self.d_in, L.in_off, L.in_cap, s[0], self.d_crc[L.c0:]))
            elif k == "build":
                L.call = ("sf_build_codes", (L.nb, self.d_fi[L.fi0:], self.d_to[L.to0 * self.tsz:]))
            elif k == "sf_enc_dev":
                if "tables_from" in L.opts:
                    T = self.L[L.opts["tables_from"]]
                    assert T.kind == "build" and T.items == L.items
                    d_tab = self.d_to[T.to0 * self.tsz:]
                else:
                    d_tab = self.d_ti[L.ti0 * self.tsz:]
                L.call = ("sf_encode_dev", (self.d_in, L.in_off, L.in_cap, s[0], d_tab, self.d_out, L.out_off, L.out_cap,
                                            self.d_n[L.n0:]))
            elif k == "sf_dec_dev":
                L.call = ("sf_decode_dev", (self.d_in, L.in_off, L.in_cap, s[0], self.d_ti[L.ti0 * self.tsz:], s[1], self.d_out,
                                            L.out_off, L.out_cap))
            else:
                raise AssertionError(k)
        self.reset()
        return self

    def _not_prefix_free(self, it):
        """the item's table with one symbol's code replaced by a proper prefix of another's; the oracle refuses it"""
        t = self.shafa.CodeTable()
        C.memmove(C.byref(t), C.byref(it.tab), C.sizeof(t))
        used = [int(s) for s in np.nonzero(it.lens)[0]]
        y = max(used, key=lambda s: it.lens[s])
        x = next(s for s in used if s != y)
        ly = int(it.lens[y])
        assert ly >= 2
        t.len[x] = ly - 1
        for q in range(32):
            t.bits[x][q] = 0
        for q in range(ly - 1):
            if (it.tab.bits[y][q >> 3] >> (7 - (q & 7))) & 1:
                t.bits[x][q >> 3] |= 0x80 >> (q & 7)
        ot = type(it.tab)()
        C.memmove(C.byref(ot), C.byref(t), C.sizeof(t))
        rc, _ = self.o.sf_decode(it.enc, ot, it.n)
        assert rc == FILE_UNRECOGNIZABLE, rc
        return t

    def reset(self):
        """every output as it is before a launch writes it (called outside a sequence only), then one synchronisation"""
        import torch
        self.d_out.fill_(FILL)
        self.d_n.fill_(SENT)
        self.d_freq.fill_(SENT)
        self.d_crc.fill_(SENT32)
        self.d_to.fill_(FILL)
        torch.cuda.synchronize()

    def max_blocks(self):
        return max(L.nb for L in self.L)

    def enqueue(self, bt, st, lo=0, hi=None):
        for L in self.L[lo:hi]:
            name, args = L.call
            getattr(bt, name)(st, *args)

    def check(self, errs, want_errs=None, relaxed=()):
        """errs: what the one finish reported.  want_errs: {block index: code}; relaxed: (launch index, block) pairs of which
        only the guard bytes are looked at.  Returns the list of problems."""
        bad, tag = [], self.name
        want_errs = want_errs or {}
        for i, e in enumerate(errs):
            if e != want_errs.get(i, 0):
                bad.append(f"{tag}: error word {i} is {e}, not {want_errs.get(i, 0)}")
        out = self.d_out.cpu().numpy()
        d_n = self.d_n.cpu().numpy()
        d_freq = self.d_freq.cpu().numpy().view(np.uint64)
        d_crc = self.d_crc.cpu().numpy().view(np.uint32)
        d_to = self.d_to.cpu().numpy()
        if not (out[:FRONT] == FILL).all():
            bad.append(f"{tag}: wrote in front of the first block")
        skip = set(relaxed)
        for r, (L, i, off, cap) in enumerate(self.regions):
            what = f"{tag}: launch {L.idx} ({L.kind}, {L.nb} blocks) block {i} ({L.items[i].name})"
            nxt = self.regions[r + 1][2] if r + 1 < len(self.regions) else off + al16(cap) + GUARD
            if not (out[off + cap:nxt] == FILL).all():
                bad.append(f"{what}: wrote behind its region, first at {off + cap + int(np.argmax(out[off + cap:nxt] != FILL))}")
            if (L.idx, i) in skip:
                continue
            w = L.want[i]
            got = out[off:off + w.size]
            if w.size > cap:
                continue                                   # a region too small on purpose: its error word is what counts
            if got.tobytes() != w.tobytes():
                bad.append(f"{what}: {first_diff(got, w)}" + (" (untouched)" if (got == FILL).all() else ""))
        for L in self.L:
            what = f"{tag}: launch {L.idx} ({L.kind}, {L.nb} blocks)"
            rel = {i for (l, i) in skip if l == L.idx}
            if hasattr(L, "n0"):
                for i in range(L.nb):
                    if i in rel or L.want[i].size > L.out_cap[i]:
                        continue
                    if int(d_n[L.n0 + i]) != L.want[i].size:
                        bad.append(f"{what} block {i}: size {int(d_n[L.n0 + i])}, not {L.want[i].size}")
                if d_n[L.n0 + L.nb] != SENT:
                    bad.append(f"{what}: wrote behind its size slots")
            if hasattr(L, "f0"):
                for i, it in enumerate(L.items):
                    want = it.hist if L.kind == "hist" else it.rle_hist
                    got = d_freq[L.f0 + i * 256:L.f0 + (i + 1) * 256]
                    if i not in rel and not (got == want).all():
                        bad.append(f"{what} block {i}: counts differ at {np.nonzero(got != want)[0][:6]}")
                if not (d_freq[L.f0 + L.nb * 256:L.f0 + L.nb * 256 + 8] == SENT).all():
                    bad.append(f"{what}: wrote behind its count slots")
            if hasattr(L, "c0"):
                for i, it in enumerate(L.items):
                    if i not in rel and int(d_crc[L.c0 + i]) != it.crc:
                        bad.append(f"{what} block {i}: CRC {int(d_crc[L.c0 + i]):08x}, not {it.crc:08x}")
                if d_crc[L.c0 + L.nb] != SENT32:
                    bad.append(f"{what}: wrote behind its CRC slots")
            if L.kind == "build":
                for i in range(L.nb):
                    got = d_to[(L.to0 + i) * self.tsz:(L.to0 + i + 1) * self.tsz].tobytes()
                    if i not in rel and got != L.want_tabs[i]:
                        bad.append(f"{what} block {i}: table differs from the host's Module T")
                if not (d_to[(L.to0 + L.nb) * self.tsz:(L.to0 + L.nb + 1) * self.tsz] == FILL).all():
                    bad.append(f"{what}: wrote behind its tables")
        return bad


def sleep_on(st):
    """about 0.1 s of one busy wave in front of the sequence: the host runs ahead of the device"""
    import torch
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)


def finish(bt, st, n):
    rc, errs = bt.finish(st, n, raise_on_error=False)
    return rc, errs


def grow_then_behind_a_sleep(seq, bt, st, n_err, want_errs=None, relaxed=(), probe=2):
    """The sequence twice on the batch, each time with one finish and a full check: first as it comes, so that the workspace,
    the parameter buffers and the ring reach their sizes (growing synchronises, which would let the device catch up), then
    behind a sleep with nothing left to grow — the host runs ahead, and `busy` tells that the stream had not drained when the
    first `probe` launches had returned.  Returns the two return codes of finish, busy and the list of problems."""
    base, bad, rcs, busy = seq.name, [], [], None
    for phase in ("growing", "behind a sleep"):
        seq.name = f"{base}, {phase}"
        if phase == "growing":
            seq.enqueue(bt, st)
        else:
            seq.reset()
            sleep_on(st)
            seq.enqueue(bt, st, 0, probe)
            busy = not st.query()
            seq.enqueue(bt, st, probe)
        rc, errs = finish(bt, st, n_err)
        rcs.append(rc)
        bad += seq.check(errs, want_errs, relaxed)
    seq.name = base
    return rcs, busy, bad


NOT_BUSY = "the stream had drained when the first calls returned: something synchronised"


def show(bad):
    return f"{len(bad)} problems:\n" + "\n".join(bad[:16])


@pytest.fixture()
def lib(shafa):
    import torch
    shafa.lib().shafa_hip_init(0)
    assert (shafa.FILE_UNRECOGNIZABLE, shafa.LACK_OF_MEMORY) == (FILE_UNRECOGNIZABLE, LACK_OF_MEMORY)
    yield shafa
    shafa.set_option("sf_decode_speculate", 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the cases
@gpu
def test_growing_batch_then_again_behind_a_busy_stream(oracle, lib, pool):
    """Cases 1 and 2.  A fresh Batch(512, 2 MiB) and one stream, no finish until the end: every entry point on 3 blocks, on 40
    blocks of 8 .. 70 KiB, on the two 1.5 MiB blocks, then sf_encode and sf_decode on 512 blocks of about 600 B — the
    workspace, both parameter buffers and the staging ring grow (the one thing that synchronises here) while earlier launches'
    results lie unread in device memory.  Then the same sequence again on the same batch behind a busy stream: nothing grows,
    so the stream must still be busy after the first round (whose staged bytes stay far below the ring's 1 MiB), and after
    the single finish every launch must be right again."""
    import torch
    plan, first = plan_growing(pool)
    seq = Sequence(lib, oracle, plan, "growing").prepare()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    bt = lib.Batch(512, 2 * MIB)
    try:
        seq.enqueue(bt, st)
        rc, errs = finish(bt, st, seq.max_blocks())
        bad = seq.check(errs)
        assert rc == 0 and not bad, show(bad)

        seq.name = "again"
        seq.reset()
        sleep_on(st)
        seq.enqueue(bt, st, 0, first)
        busy = not st.query()
        seq.enqueue(bt, st, first)
        rc, errs = finish(bt, st, seq.max_blocks())
        bad = seq.check(errs)
        assert busy, "the stream had drained when the first round's calls returned: something synchronised"
        assert rc == 0 and not bad, show(bad)
    finally:
        bt.close()


@gpu
@pytest.mark.parametrize("speculate", [2, 0])
def test_every_entry_point_right_after_every_other(oracle, lib, pool, speculate):
    """Case 3.  One batch and one stream, once while the batch grows and once behind a sleep: after an rle_encode of a 1.5 MiB block (a large, dirty workspace) every
    ordered pair of hist256, rle_encode, sf_encode, sf_decode, rle_decode, crc32_dev, sf_build_codes + sf_encode_dev and
    sf_decode_dev is adjacent once, on 3 .. 6 small blocks, so every launcher runs on what every other left in the workspace;
    sf_decode_speculate 2 (every block speculates, the fall-back included) and 0 (the exact kernels)."""
    import torch
    plan = plan_pairs(pool)
    e = entries_of(plan)
    assert {(a, b) for a in ENTRIES for b in ENTRIES} <= set(zip(e, e[1:]))
    seq = Sequence(lib, oracle, plan, f"pairs/spec{speculate}").prepare()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    bt = lib.Batch(8, 2 * MIB)
    try:
        lib.set_option("sf_decode_speculate", speculate)
        rcs, busy, bad = grow_then_behind_a_sleep(seq, bt, st, seq.max_blocks())
        assert rcs == [0, 0] and not bad, show(bad)
        assert busy, NOT_BUSY
    finally:
        lib.set_option("sf_decode_speculate", 1)
        bt.close()


@gpu
def test_staging_ring_wraps_with_copies_pending(oracle, lib, pool):
    """Case 4.  Once while the batch grows, then behind a sleep: 32 launches in turn of sf_encode (512 blocks of about 600 B: more than 512 KiB of tables) and
    sf_decode (48 blocks of 8 .. 40 KiB with 48 different tables), each with another permutation: they ask the staging ring
    for more than twice its size (test_sequence_shapes), so regions are handed out again while the copies from them are
    pending — a table overwritten before its copy ran shows in that launch's blocks."""
    import torch
    seq = Sequence(lib, oracle, plan_ring(pool), "ring").prepare()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    bt = lib.Batch(512, 64 * KIB)
    try:
        rcs, busy, bad = grow_then_behind_a_sleep(seq, bt, st, seq.max_blocks())
        assert rcs == [0, 0] and not bad, show(bad)
        assert busy, NOT_BUSY
    finally:
        bt.close()


@gpu
def test_parameter_buffers_inline_and_side_stream(oracle, lib, pool):
    """Case 5.  Once while the batch grows, then behind a sleep: sf_encode / sf_decode / sf_encode_dev / sf_decode_dev launches whose parameters lie below
    PARAMS_INLINE_BYTES (S: 2 blocks, copied in the launch's stream) or above it (L: 64 blocks, copied on the side stream)
    in the order S L S S L L S L L L S S S L: each of the two device buffers is written both ways, after a reader of either
    kind.  Then rle_encode and rle_decode of 600 blocks (batch_upload's copy kernel) between launches of 3 (its
    hipMemcpyAsync).  The sides are proved in test_sequence_shapes."""
    import torch
    seq = Sequence(lib, oracle, plan_params(pool), "params").prepare()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    bt = lib.Batch(600, 64 * KIB)
    try:
        rcs, busy, bad = grow_then_behind_a_sleep(seq, bt, st, seq.max_blocks())
        assert rcs == [0, 0] and not bad, show(bad)
        assert busy, NOT_BUSY
    finally:
        bt.close()


@gpu
def test_errors_in_the_middle_of_a_sequence(oracle, lib, pool):
    """Case 6.  Ten launches of 8 blocks, one finish(st, 8); once while the batch grows, then behind a sleep.  Launch 4 (sf_decode): block 3's stream cut in half, which the
    oracle calls FILE_UNRECOGNIZABLE; launch 6 (sf_decode): block 5's table not prefix-free (refused on the host); launch 7
    (sf_encode): block 1's region half of what it needs, LACK_OF_MEMORY.  The error words must be exactly these three, at 3, 5
    and 1; every block must be right except those with index 3, 5 or 1 in the launch that set the word and behind it (the
    header promises nothing for them: their guard bytes only).  A second finish reports zeros, and a further launch on the
    batch finishes clean."""
    import torch
    group = pool.small + pool.mid[:5]
    kinds = ["hist", "rle_enc_f", "sf_enc", "rle_dec", "sf_dec", "crc", "sf_dec", "sf_enc", "sf_dec_dev", "sf_enc_dev"]
    opts = {4: dict(cut=(3,)), 6: dict(bad_table=(5,)), 7: dict(small_cap=(1,))}
    plan = []
    for k, kind in enumerate(kinds):
        add(plan, kind, pick(group, 8, k), **opts.get(k, {}))
    assert len(plan) == 10
    cut = plan[4][1][3]
    rc, _ = oracle.sf_decode(cut.enc[:cut.enc.size // 2], cut.tab, cut.n)
    assert rc == FILE_UNRECOGNIZABLE
    relaxed = [(l, 3) for l in range(4, 10)] + [(l, 5) for l in range(6, 10)] + [(l, 1) for l in range(7, 10)]
    seq = Sequence(lib, oracle, plan, "errors").prepare()
    after = Sequence(lib, oracle, [("sf_dec", pick(group, 8, 30), {}), ("rle_enc", pick(group, 8, 31), {})], "after").prepare()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    bt = lib.Batch(8, 64 * KIB)
    try:
        rcs, busy, bad = grow_then_behind_a_sleep(seq, bt, st, 8, {3: FILE_UNRECOGNIZABLE, 5: FILE_UNRECOGNIZABLE,
                                                                   1: LACK_OF_MEMORY}, relaxed)
        rc2, errs2 = finish(bt, st, 8)
        assert not bad, show(bad)
        assert rcs == [LACK_OF_MEMORY] * 2, rcs                    # the first error by block index: block 1's
        assert busy, NOT_BUSY
        assert rc2 == 0 and errs2 == [0] * 8, (rc2, errs2)
        after.enqueue(bt, st)
        rc, errs = finish(bt, st, 8)
        bad = after.check(errs)
        assert rc == 0 and not bad, show(bad)
    finally:
        bt.close()


@gpu
def test_batch_changes_stream(oracle, lib, pool):
    """Case 7.  One batch on s1, s2, then s1 again: a sleep and an sf_decode of 40 blocks on s1, at once an rle_encode of 40
    other blocks on s2 — "a launch on another stream first waits for the batch's previous stream", so s1 has drained when that
    call returns (the one synchronisation of this case) — then an sf_encode on s1 and finish(s1)."""
    import torch
    group = pool.mid + pool.large
    plan = []
    add(plan, "sf_dec", pick(group, 40, 3))
    add(plan, "rle_enc_f", pick(group, 40, 8))
    add(plan, "sf_enc", pick(group, 40, 14))
    seq = Sequence(lib, oracle, plan, "streams").prepare()
    dev = torch.device("cuda", 0)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    bt = lib.Batch(40, 128 * KIB)
    try:
        sleep_on(s1)
        seq.enqueue(bt, s1, 0, 1)
        seq.enqueue(bt, s2, 1, 2)
        drained = s1.query()
        seq.enqueue(bt, s1, 2, 3)
        rc, errs = finish(bt, s1, 40)
        bad = seq.check(errs)
        assert drained, "the launch on s2 returned while the batch's work on s1 was still running"
        assert rc == 0 and not bad, show(bad)
    finally:
        bt.close()
