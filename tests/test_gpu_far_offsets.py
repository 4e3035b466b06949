"""Block offsets past 4 GiB in the device entry points (include/shafa_hip.h: "the offsets are 64-bit").

Every test here runs ONE call several times on the same bytes and moves only where they lie: every side near, every side far,
and each side far on its own, which names the culprit.  A far run has to equal the near run byte for byte (outputs, sizes, error
words, return code) and, directly, the independent reference of the file that owns the family.

The arena is one uint8 allocation of 2^32 + 512 MiB, and every side of a call takes its base pointer: where a byte lies is
decided by the offset alone.  Near regions lie in [0, 128 MiB), far regions at o = 2^32 + s with s in [128 MiB, 256 MiB).  Bit 31 of
o is clear, so both 32-bit misreadings of o (zero- and sign-extended) give s = o - 2^32, the region's SHADOW, inside the arena and
never on a near region.  Before a far call the shadow of an output holds 0xEE and the shadow of an input holds decoy bytes that
differ from the input in every byte; afterwards the 64 guard bytes on both sides of every output still hold their fill and the
low 512 MiB equal a clone taken before the call (near outputs put back first).  A truncated offset therefore shows as wrong bytes
or as a touched shadow, with the side's name in the message, and not as a fault.

    entry point                         sides moved far                reference
    hist256, hist256_tiles              in, thist                      numpy bincount per block and per 32 KiB tile
    rle_encode, rle_encode_tiles        in, out, thist                 oracle rle_encode, bincount of its bytes (one block short of room)
    rle_decode, rle_decode_dev          in, out                        oracle rle_decode (one block short of room)
    rle_decoded_size_dev                in                             oracle rle_decode
    rle_encoded_size_dev, _hist_dev     in                             oracle rle_encode, bincount of its bytes
    sf_encode, _tiles, _dev             in, out, thist                 oracle sf_encode; Lmax <= 8, <= 12, 13..15, 16, 17..32, > 32 in
                                                                       each; one block without a code, one short of room in each
    sf_decode, sf_decode_dev            in, out                        the encoder's input, the same six forms
    compare_dev                         a, ref (+5, +11)               numpy: first differing index
    crc32_dev                           in (+5, +11)                   zlib.crc32
    find_dev                            in (+5, +11)                   bytes.find
    split/merge_planes_dev              el (+5, +11), planes           numpy transpose
    split/merge_planes_xor_dev          el, base (+5, +11), planes     numpy transpose of the XOR
    split/merge_planes_diff_dev         el (+5, +11), planes           test_gpu_planes_grid._z_planes at lags (1,)
    split/merge_planes_lag_dev          el, planes                     test_gpu_planes_grid._z_planes at lags (L,)
    split/merge_planes_grid_dev         el, planes                     test_gpu_planes_grid._z_planes / _x_bytes
    hist_planes_grid_dev                in                             test_planes_grid_hist_cpu.plane_histograms
    split_planes_grid_quant / _round    el, planes, outl (its pointer) test_gpu_fields._model / test_gpu_rounding._rule, _z_planes
    merge_planes_grid_quant / _round    planes, outl (pointer), el     the models' restored bits
    hist_planes_grid_quant / _round     in                             bincount of the models' planes, the models' outlier counts
    error_dev, _quant_dev, _round_dev   x (the original), a            test_gpu_grid_walks.exact_record, all twelve words
    split/merge_records_dev             rec (+5, +11), cols            numpy reshape, widths 3 and 17
    seek_index_dev                      in                             the header's checkpoints: sums of code lengths
    read_spans_dev                      pay (+5, +11), out             slices of the encoder's input
    pack_payloads, _files               src, dst (+5, +11)             test_gpu_pack._payload_file's statement, both framings
    pack_cod, pack_freq, _files         dst (+5, +11)                  the host formatter's text in test_gpu_pack._text_file's frame
    the three _files packs              src, dst (+5, +11)             the middle file of three one byte short of room
    unpack_shaf, unpack_payloads, _at,  file (+5, +11), dst            the file's layout computed on the host; through _files and
    unpack_shaf_files                                                  _at the payload places themselves are past 2^32
    unpack_payloads, _at                file (+5, +11), dst            one payload's region 16 bytes short
    unpack_cod, unpack_freq,            text (+5, +11)                 the tables, counts, sizes and places that went into the host
    unpack_rle_freq, _files                                            formatter's text

crc32_combine_dev, sf_build_codes and sf_encoded_size_dev take no offsets and no byte region, so they have no far side.

rle_encode(_tiles), sf_encode and sf_decode(_dev) run under the defaults and under each set of test_gpu_codec.OPTION_SETS: every
encoder and decoder path the library can be told to take has its own address arithmetic.

test_far_cpu.py runs every test of this file on DryArena, which makes and checks the placements without a device."""
import contextlib
import zlib

import numpy as np
import pytest

from test_gpu_codec import DEFAULT_OPTIONS, OPTION_SETS, option_id

pytestmark = pytest.mark.gpu

G = 1 << 32
LOW = 512 << 20                     # the part of the arena a 32-bit misreading can reach, compared after every call
ARENA_BYTES = G + LOW
NEAR = (0, 128 << 20)               # near regions
SHADOW = (128 << 20, 256 << 20)     # shadows of the far regions [G + SHADOW[0], G + SHADOW[1])
GUARD = 64
FILL, SHADOW_FILL = 0xA5, 0xEE
SHIFTS = (0, 5, 11)
DEV = "cuda:0"
TILE = 8192


def al16(x):
    return (x + 15) // 16 * 16


class Side:
    """One side of a call: `regions` are uint8 arrays (an input side) or lengths (an output side), one per block or plane.
    exact: nothing past a region's own bytes may be written (otherwise: past its bytes rounded up to 16); any_align: the
    header promises any byte alignment for this side, so the shifted runs move it."""

    def __init__(self, name, regions, out=False, exact=False, any_align=False):
        self.name, self.regions, self.out, self.exact, self.any_align = name, list(regions), out, exact, any_align


def place(sides, far, shift=0):
    """{side: [(offset, bytes, room)]}: a bump allocation with GUARD bytes on both sides of every region, near sides from
    NEAR[0], far sides at G + (a bump from SHADOW[0]); no torch, so that the arithmetic is checked without a device"""
    pos = {False: NEAR[0] + 4096, True: SHADOW[0] + 4096}
    out = {}
    for s in sides:
        sh = shift if s.any_align else 0
        is_far = s.name in far
        rows = []
        for r in s.regions:
            n = int(r) if isinstance(r, (int, np.integer)) else int(r.size)
            room = n if (s.exact or sh) else al16(n)
            o = al16(pos[is_far]) + GUARD + sh
            pos[is_far] = o + room + GUARD
            rows.append((o + (G if is_far else 0), n, room))
        out[s.name] = rows
    assert pos[False] <= NEAR[1] and pos[True] <= SHADOW[1], "the case does not fit the arena's windows"
    return out


def misreadings(o):
    """what a 32-bit slip makes of offset o: zero-extended and sign-extended"""
    lo = o & 0xFFFFFFFF
    return lo, lo - (1 << 32) if lo >> 31 else lo


def check_layout(lay):
    """the arena's rule for one layout: near regions in NEAR, far regions at G + their shadow in SHADOW with bit 31 clear, so that
    both misreadings of a far offset give the shadow; regions, shadows and their guards pairwise disjoint and inside LOW"""
    spans = []
    for name, rows in lay.items():
        for o, n, room in rows:
            if o >= G:
                assert not o >> 31 & 1, (name, o)
                assert misreadings(o) == (o - G, o - G), (name, o)
                assert o + room + GUARD <= ARENA_BYTES
                lo, hi = o - G - GUARD, o - G + room + GUARD
                assert SHADOW[0] <= lo and hi <= SHADOW[1], (name, o)
            else:
                lo, hi = o - GUARD, o + room + GUARD
                assert NEAR[0] <= lo and hi <= NEAR[1], (name, o)
            spans.append((lo, hi, name))
    spans.sort()
    for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
        assert hi <= lo, (a, b)
    assert NEAR[1] <= SHADOW[0] and SHADOW[1] <= LOW


class Arena:
    dry = False

    def __init__(self):
        import torch
        self.torch = torch
        free, total = torch.cuda.mem_get_info()
        need = ARENA_BYTES + 2 * LOW + (1 << 30)
        if free < need:
            pytest.skip(f"the arena needs {need} bytes of device memory, {free} are free")
        self.buf = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=DEV)
        self.buf[:LOW].fill_(FILL)
        assert self.buf.data_ptr() % 16 == 0

    def close(self):
        self.buf = None
        self.torch.cuda.empty_cache()

    def run(self, sides, far, call, shift=0, label=""):
        """place the sides, fill shadows and guards, run call({side: [offsets]}) and check that nothing but the outputs changed
        -> call's dict plus "out": {side: [the bytes of each region]}"""
        torch, buf = self.torch, self.buf
        lay = place(sides, far, shift)
        check_layout(lay)
        rng = np.random.default_rng(20261021)
        for s in sides:
            for (o, n, room), r in zip(lay[s.name], s.regions):
                if s.out:
                    buf[o - GUARD:o + room + GUARD] = FILL
                    if o >= G:
                        buf[o - G - GUARD:o - G + room + GUARD] = SHADOW_FILL
                elif n:
                    buf[o:o + n] = torch.from_numpy(np.array(r, copy=True)).to(DEV)
                    if o >= G:                                             # decoy: differs from the input in every byte
                        decoy = r + rng.integers(1, 256, n, dtype=np.uint8)
                        buf[o - G:o - G + n] = torch.from_numpy(decoy).to(DEV)
        snap = buf[:LOW].clone()
        torch.cuda.synchronize()
        res = dict(call({s.name: [o for o, _, _ in lay[s.name]] for s in sides}))
        torch.cuda.synchronize()
        outs = {}
        for s in sides:
            if not s.out:
                continue
            got = []
            for b, (o, n, room) in enumerate(lay[s.name]):
                got.append(buf[o:o + n].cpu().numpy())
                for lo, hi, where in ((o - GUARD, o, "in front of"), (o + room, o + room + GUARD, "behind")):
                    assert bool((buf[lo:hi] == FILL).all()), f"{label}: the guard bytes {where} region {b} of side '{s.name}' were written"
                if o < G:
                    buf[o:o + room] = snap[o:o + room]
            outs[s.name] = got
        if not torch.equal(buf[:LOW], snap):
            at = int((buf[:LOW] != snap).nonzero()[0])
            who = [f"the shadow of region {b} of far side '{s.name}'" for s in sides for b, (o, n, room) in enumerate(lay[s.name])
                   if o >= G and o - G - GUARD <= at < o - G + room + GUARD]
            pytest.fail(f"{label}: byte {at} of the arena changed, {who[0] if who else 'which is no region of this call'}: "
                        "an offset was cut to 32 bits")
        res["out"] = outs
        return res


@pytest.fixture(scope="module")
def arena():
    a = Arena()
    yield a
    a.close()


def _canon(v):
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (list, tuple)):
        return tuple(_canon(x) for x in v)
    return v


def _outputs(res):
    """the outputs' bytes, cut to what the call says it produced (res["used"]: {side: [bytes]}) where it says so"""
    used = res.get("used", {})
    return {(s, b): r[:used[s][b]] if s in used else r for s, rows in res["out"].items() for b, r in enumerate(rows)}


def same(near, got, label):
    for k in near:
        if k not in ("out", "used"):
            assert _canon(near[k]) == _canon(got[k]), f"{label}: '{k}' differs from the near run: {got[k]} vs {near[k]}"
    a, b = _outputs(near), _outputs(got)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), f"{label}: region {key[1]} of side '{key[0]}' differs from the near run"


def drive(arena, sides, call, check):
    names = [s.name for s in sides]
    runs = [("every side far", set(names), 0)]
    if len(names) > 1:
        runs += [(f"only side '{s}' far", {s}, 0) for s in names]
    if any(s.any_align for s in sides):
        runs += [(f"every side far, + {d} bytes", set(names), d) for d in SHIFTS[1:]]
    if arena.dry:                                                          # test_far_cpu.py: the placements alone, no device
        for label, far, shift in [("every side near", (), 0)] + runs:
            arena.run(sides, far, call, shift, label)
        return
    near = arena.run(sides, (), call, label="every side near")
    check(near, "every side near")
    failures = []                                                          # every run is made: the one-side runs name the culprit
    for label, far, shift in runs:
        try:
            got = arena.run(sides, far, call, shift, label)
            same(near, got, label)
            check(got, label)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(str(e).split("\n")[0][:400])
    assert not failures, "\n".join(failures)


class DryArena:
    """the arena without a device: every placement a case asks for is made and checked, nothing runs"""
    dry = True

    def __init__(self):
        self.layouts = []

    def run(self, sides, far, call, shift=0, label=""):
        lay = place(sides, far, shift)
        check_layout(lay)
        self.layouts.append((label, lay))


def batch_call(shafa, nb, max_bytes, body):
    """body(batch, stream) on a fresh batch, then finish -> (return code, error words)"""
    import torch
    st = torch.cuda.Stream(device=DEV)
    bt = shafa.Batch(nb, max(int(max_bytes), 16))
    try:
        torch.cuda.synchronize()
        body(bt, st)
        rc, errs = bt.finish(st, nb, raise_on_error=False)
    finally:
        bt.close()
    return rc, errs


def i64(v, fill=None):
    import torch
    if fill is not None:
        return torch.full((v,), fill, dtype=torch.int64, device=DEV)
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=DEV)


def host(t):
    return t.cpu().numpy()


def tile_hist(b):
    """[tiles of 32 KiB, 256] uint16 counts: what hist256_tiles leaves for a block (test_gpu_rle_grid._tile_hist)"""
    from test_gpu_rle_grid import _tile_hist
    return _tile_hist(b)


def hist(b):
    return np.bincount(b, minlength=256).astype(np.int64)


def zipf(shafa, oracle, seed, n):
    return oracle.gen_bytes(seed, n, shafa.zipf_table(1.2)) if n else np.zeros(0, np.uint8)


SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 0, 32768 + 1]         # 1 B, a tile -1 / +1, tiles and a ragged tail, empty


# ---------------------------------------------------------------- hist256, hist256_tiles
@pytest.mark.parametrize("tiles", [False, True], ids=["hist256", "hist256_tiles"])
def test_hist256(arena, shafa, oracle, tiles):
    blocks = [zipf(shafa, oracle, 50 + i, n) for i, n in enumerate(SIZES)]
    nb = len(blocks)
    sides = [Side("in", blocks)]
    if tiles:
        sides.append(Side("thist", [shafa.tile_hist_bytes(n) for n in SIZES], out=True))

    def call(off):
        d_freq = i64(nb * 256, fill=-1)
        if tiles:
            body = lambda bt, st: bt.hist256_tiles(st, arena.buf, off["in"], SIZES, d_freq, arena.buf, off["thist"])
        else:
            body = lambda bt, st: bt.hist256(st, arena.buf, off["in"], SIZES, d_freq)
        rc, errs = batch_call(shafa, nb, max(SIZES), body)
        return dict(rc=rc, errs=errs, freq=host(d_freq).reshape(nb, 256))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, blk in enumerate(blocks):
            assert np.array_equal(res["freq"][b], hist(blk)), f"{label}: histogram of block {b}"
            if tiles:
                t = tile_hist(blk)
                assert res["out"]["thist"][b][:t.size * 2].tobytes() == t.tobytes(), f"{label}: tile histograms of block {b}"

    drive(arena, sides, call, check)


# ---------------------------------------------------------------- the codec's option sets
CODEC_OPTIONS = [{}] + OPTION_SETS                                         # the defaults, then every set of test_gpu_codec


def codec_id(o):
    return option_id(o) or "default"


@contextlib.contextmanager
def options_set(shafa, options):
    shafa.lib().shafa_hip_init(0)
    for k, v in options.items():
        shafa.set_option(k, v)
    try:
        yield
    finally:
        for k, v in DEFAULT_OPTIONS.items():
            shafa.set_option(k, v)


# ---------------------------------------------------------------- RLE
def rle_raw():
    from test_gpu_rle_grid import _raw
    sizes = [TILE * k + 5 for k in (1, 3, 2, 0)] + [3 * 4096, 0, 1]
    return [_raw(400 + i, n) if n else np.zeros(0, np.uint8) for i, n in enumerate(sizes)]


def rle_streams(oracle):
    from test_gpu_rle_grid import _rle_input
    return [_rle_input(oracle, 300 + i, t) for i, t in enumerate((1, 3, 2, 0, 5))]


def rle_encode_family(arena, shafa, oracle, tiles, short=None):
    """rle_encode / rle_encode_tiles over rle_raw; short: a block whose region holds half of its RLE bytes"""
    blocks = rle_raw()
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    caps = [2 * n + 16 for n in sizes]
    want = [oracle.rle_encode(b) if b.size else np.zeros(0, np.uint8) for b in blocks]
    if short is not None:
        caps[short] = want[short].size // 2 // 16 * 16
    expect = {} if short is None else {short: shafa.LACK_OF_MEMORY}
    sides = [Side("in", blocks), Side("out", caps, out=True)]
    if tiles:
        sides.append(Side("thist", [shafa.tile_hist_bytes(c) for c in caps], out=True))

    def call(off):
        d_n, d_freq = i64(nb, fill=-1), i64(nb * 256, fill=-1)
        if tiles:
            body = lambda bt, st: bt.rle_encode_tiles(st, arena.buf, off["in"], sizes, arena.buf, off["out"], caps, d_n, d_freq,
                                                      arena.buf, off["thist"])
        else:
            body = lambda bt, st: bt.rle_encode(st, arena.buf, off["in"], sizes, arena.buf, off["out"], caps, d_n, d_freq)
        rc, errs = batch_call(shafa, nb, max(caps), body)
        n = [int(x) for x in host(d_n)]
        used = {"out": [0 if e else min(max(x, 0), c) for x, e, c in zip(n, errs, caps)]}
        if tiles:
            used["thist"] = [0 if e else tile_hist(w).size * 2 for w, e in zip(want, errs)]
        freq = host(d_freq).reshape(nb, 256)
        freq[np.array(errs) != 0] = -1                                     # a refused block's counts are not defined
        return dict(rc=rc, errs=errs, n=n, freq=freq, used=used)

    def check(res, label):
        assert (res["rc"] == 0) == (not expect), label
        for b, w in enumerate(want):
            assert res["errs"][b] == expect.get(b, 0), f"{label}: error word of block {b}"
            if b in expect:
                continue
            assert res["n"][b] == w.size and res["out"]["out"][b][:w.size].tobytes() == w.tobytes(), f"{label}: RLE bytes of block {b}"
            assert np.array_equal(res["freq"][b], hist(w)), f"{label}: histogram of block {b}"
            if tiles:
                t = tile_hist(w)
                assert res["out"]["thist"][b][:t.size * 2].tobytes() == t.tobytes(), f"{label}: tile histograms of block {b}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("options", CODEC_OPTIONS, ids=codec_id)
@pytest.mark.parametrize("tiles", [False, True], ids=["rle_encode", "rle_encode_tiles"])
def test_rle_encode(arena, shafa, oracle, tiles, options):
    with options_set(shafa, options):
        rle_encode_family(arena, shafa, oracle, tiles)


@pytest.mark.parametrize("tiles", [False, True], ids=["rle_encode", "rle_encode_tiles"])
def test_rle_encode_one_block_short_of_room(arena, shafa, oracle, tiles):
    """block 1 (three tiles and a tail) has half the room its RLE bytes need: LACK_OF_MEMORY for it alone, its neighbours whole,
    nothing behind its region"""
    rle_encode_family(arena, shafa, oracle, tiles, short=1)


@pytest.mark.parametrize("dev", [False, True], ids=["rle_decode", "rle_decode_dev"])
def test_rle_decode_one_block_short_of_room(arena, shafa, oracle, dev):
    """block 2 has half the room it needs: LACK_OF_MEMORY for it alone, its neighbours whole, nothing behind its region"""
    blocks = rle_streams(oracle)
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    full = [oracle.rle_decode(b) for b in blocks]
    assert all(rc == 0 for rc, _ in full)
    caps = [w.size for _, w in full]
    caps[2] = caps[2] // 2 // 16 * 16
    want = [oracle.rle_decode(b, cap=c) for b, c in zip(blocks, caps)]
    assert want[2][0] == shafa.LACK_OF_MEMORY
    sides = [Side("in", blocks), Side("out", caps, out=True)]

    def call(off):
        d_n = i64(nb, fill=-1)
        if dev:
            d_sizes = i64(sizes)
            body = lambda bt, st: bt.rle_decode_dev(st, arena.buf, off["in"], sizes, d_sizes, arena.buf, off["out"], caps, d_n)
        else:
            body = lambda bt, st: bt.rle_decode(st, arena.buf, off["in"], sizes, arena.buf, off["out"], caps, d_n)
        rc, errs = batch_call(shafa, nb, max(sizes + caps), body)
        n = [int(x) for x in host(d_n)]
        return dict(rc=rc, errs=errs, n=n, used={"out": [0 if e else x for x, e in zip(n, errs)]})

    def check(res, label):
        assert res["rc"] == shafa.LACK_OF_MEMORY, label
        for b, (rc, w) in enumerate(want):
            assert res["errs"][b] == rc, f"{label}: error word of block {b}"
            if rc == 0:
                assert res["n"][b] == w.size and res["out"]["out"][b].tobytes() == w.tobytes(), f"{label}: decoded bytes of block {b}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("entry", ["rle_decoded_size_dev", "rle_encoded_size_dev", "rle_encoded_hist_dev"])
def test_rle_size_passes(arena, shafa, oracle, entry):
    if entry == "rle_decoded_size_dev":
        blocks = rle_streams(oracle)
        want = [oracle.rle_decode(b)[1] for b in blocks]
    else:
        blocks = rle_raw()
        want = [oracle.rle_encode(b) if b.size else np.zeros(0, np.uint8) for b in blocks]
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    sides = [Side("in", blocks)]

    def call(off):
        d_n, d_freq, d_sizes = i64(nb, fill=-1), i64(nb * 256, fill=-1), i64(sizes)
        if entry == "rle_encoded_hist_dev":
            body = lambda bt, st: bt.rle_encoded_hist_dev(st, arena.buf, off["in"], sizes, d_sizes, d_n, d_freq)
        else:
            body = lambda bt, st: getattr(bt, entry)(st, arena.buf, off["in"], sizes, d_sizes, d_n)
        rc, errs = batch_call(shafa, nb, max(sizes), body)
        return dict(rc=rc, errs=errs, n=[int(x) for x in host(d_n)], freq=host(d_freq).reshape(nb, 256))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        assert res["n"] == [w.size for w in want], label
        if entry == "rle_encoded_hist_dev":
            for b, w in enumerate(want):
                assert np.array_equal(res["freq"][b], hist(w)), f"{label}: histogram of block {b}"

    drive(arena, sides, call, check)


# ---------------------------------------------------------------- Shannon-Fano
FORMS = ("lmax8", "lmax12", "lmax13_15", "lmax16", "lmax17_32", "lmax33")


def sf_case(shafa, oracle, form):
    """blocks and oracle tables of one code-length form of sf_encode, at 1 B, a tile - 1 / + 1 and three tiles with a tail"""
    from test_gpu_parity import long_code_case
    cuts = (1, TILE - 1, TILE + 1, 3 * TILE + 5, 32768 * 2 + 77)
    if form == "lmax8":
        data = (oracle.gen_bytes(920, cuts[-1]) % 5).astype(np.uint8) * 50
        tab = oracle.sf_build(oracle.hist256(data))
        lo, hi = 1, 8
    else:
        nsyms, seed, lo, hi = {"lmax12": (13, 8, 9, 12), "lmax13_15": (14, 6, 13, 15), "lmax16": (17, 3, 16, 16),
                               "lmax17_32": (30, 9, 17, 32), "lmax33": (60, 10, 33, 255)}[form]
        tab, data = long_code_case(oracle, cuts[-1], nsyms, 0.5, seed)
    assert lo <= int(tab.lens().max()) <= hi, (form, int(tab.lens().max()))
    return [np.ascontiguousarray(data[:n]) for n in cuts], [tab] * len(cuts)


def table_bytes(shafa, tables):
    import torch
    from test_gpu_parity import to_shafa_table
    arr = shafa.Batch._tables([to_shafa_table(shafa, t) for t in tables])
    return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


def encode_family(arena, shafa, oracle, blocks, tables, entry, caps=None, expect=None):
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    want = [oracle.sf_encode(b, t) for b, t in zip(blocks, tables)]
    caps = caps or [((w.size + 15) // 16 + 1) * 16 for _, w in want]
    expect = expect or {}
    tarr, d_tables = table_bytes(shafa, tables)
    sides = [Side("in", blocks), Side("out", caps, out=True)]
    if entry == "sf_encode_tiles":
        sides.append(Side("thist", [tile_hist(b).reshape(-1).view(np.uint8) for b in blocks]))

    def call(off):
        d_n = i64(nb, fill=-1)
        if entry == "sf_encode":
            body = lambda bt, st: bt.sf_encode(st, arena.buf, off["in"], sizes, tarr, arena.buf, off["out"], caps, d_n)
        elif entry == "sf_encode_tiles":
            body = lambda bt, st: bt.sf_encode_tiles(st, arena.buf, off["in"], sizes, tarr, arena.buf, off["thist"], arena.buf,
                                                     off["out"], caps, d_n)
        else:
            d_sizes = i64(sizes)
            body = lambda bt, st: bt.sf_encode_dev(st, arena.buf, off["in"], sizes, d_sizes, d_tables, arena.buf, off["out"], caps, d_n)
        rc, errs = batch_call(shafa, nb, max(sizes + caps), body)
        n = [int(x) for x in host(d_n)]
        return dict(rc=rc, errs=errs, n=n, used={"out": [0 if e else min(max(x, 0), c) for x, e, c in zip(n, errs, caps)]})

    def check(res, label):
        for b, (rc, w) in enumerate(want):
            assert res["errs"][b] == expect.get(b, 0), f"{label}: error word of block {b}"
            if b not in expect:
                assert rc == 0 and res["n"][b] == w.size and res["out"]["out"][b][:w.size].tobytes() == w.tobytes(), \
                    f"{label}: code bytes of block {b}"
        assert (res["rc"] == 0) == (not expect), label

    drive(arena, sides, call, check)


@pytest.mark.parametrize("options", CODEC_OPTIONS, ids=codec_id)
@pytest.mark.parametrize("form", FORMS)
def test_sf_encode(arena, shafa, oracle, form, options):
    blocks, tables = sf_case(shafa, oracle, form)
    with options_set(shafa, options):
        encode_family(arena, shafa, oracle, blocks, tables, "sf_encode")


@pytest.mark.parametrize("entry", ["sf_encode_tiles", "sf_encode_dev"])
@pytest.mark.parametrize("form", FORMS)
def test_sf_encode_tiles_and_dev(arena, shafa, oracle, form, entry):
    blocks, tables = sf_case(shafa, oracle, form)
    encode_family(arena, shafa, oracle, blocks, tables, entry)


@pytest.mark.parametrize("entry,one_pass", [("sf_encode", 1), ("sf_encode", 1 << 20), ("sf_encode_tiles", 0), ("sf_encode_dev", 0)],
                         ids=["sf_encode-one_pass", "sf_encode-three_kernels", "sf_encode_tiles", "sf_encode_dev"])
def test_sf_encode_errors_stay_with_their_block(arena, shafa, oracle, entry, one_pass):
    """test_gpu_encode_onepass.test_one_pass_error_semantics: block 2 holds a symbol without a code, block 4 has half the room"""
    from test_gpu_encode_onepass import zipf_blocks
    blocks, tables = zipf_blocks(shafa, oracle, [50000] * 6, seed0=700)
    f = oracle.hist256(blocks[2])
    blocks[2] = blocks[2].copy()
    blocks[2][12345] = 250
    f[250] = 0
    tables[2] = oracle.sf_build(f)
    assert tables[2].lens()[250] == 0
    need = [oracle.sf_encode(b, t)[1].size for b, t in zip(blocks, tables)]
    caps = [((w + 15) // 16 + 1) * 16 for w in need]
    caps[4] = (need[4] // 2) // 16 * 16
    with options_set(shafa, {"sf_encode_one_pass_min_blocks": one_pass}):
        encode_family(arena, shafa, oracle, blocks, tables, entry, caps=caps,
                      expect={2: shafa.FILE_UNRECOGNIZABLE, 4: shafa.LACK_OF_MEMORY})


@pytest.mark.parametrize("options", CODEC_OPTIONS, ids=codec_id)
@pytest.mark.parametrize("entry", ["sf_decode", "sf_decode_dev"])
@pytest.mark.parametrize("form", FORMS)
def test_sf_decode(arena, shafa, oracle, form, entry, options):
    """the streams are the oracle's; the forms up to 16 bits leave through the symbol pass's buffer-resource stores"""
    blocks, tables = sf_case(shafa, oracle, form)
    if form == "lmax33" and entry == "sf_decode_dev":                      # codes of 33..64 bits have one slot a call (the header)
        blocks, tables = blocks[3:4], tables[3:4]
    nb = len(blocks)
    streams = []
    for b, t in zip(blocks, tables):
        rc, e = oracle.sf_encode(b, t)
        assert rc == 0
        streams.append(e)
    sizes, nsym = [e.size for e in streams], [b.size for b in blocks]
    tarr, d_tables = table_bytes(shafa, tables)
    sides = [Side("in", streams), Side("out", nsym, out=True)]

    def call(off):
        if entry == "sf_decode":
            body = lambda bt, st: bt.sf_decode(st, arena.buf, off["in"], sizes, tarr, nsym, arena.buf, off["out"])
        else:
            d_sizes, d_nsym = i64(sizes), i64(nsym)
            body = lambda bt, st: bt.sf_decode_dev(st, arena.buf, off["in"], sizes, d_sizes, d_tables, d_nsym, arena.buf, off["out"], nsym)
        rc, errs = batch_call(shafa, nb, max(sizes + nsym), body)
        return dict(rc=rc, errs=errs)

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, blk in enumerate(blocks):
            assert res["out"]["out"][b].tobytes() == blk.tobytes(), f"{label}: decoded bytes of block {b}"

    with options_set(shafa, options):
        drive(arena, sides, call, check)


# ---------------------------------------------------------------- readers
def test_compare_dev(arena, shafa):
    rng = np.random.default_rng(31)
    lens = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 3 * TILE + 5, 2 * TILE]
    ref = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    a = [r.copy() for r in ref]
    a[3][TILE - 1] ^= 1                                                    # the last byte
    a[5][2 * TILE + 7] ^= 0x80
    a[6][5] ^= 1
    a[6][TILE + 7] ^= 1                                                    # two differences: the first wins
    a[7] = a[7][:TILE + 3]                                                 # unequal sizes: the smaller one
    nb = len(lens)
    an = [x.size for x in a]
    want = []
    for x, r in zip(a, ref):
        m = min(x.size, r.size)
        d = np.nonzero(x[:m] != r[:m])[0]
        want.append(int(d[0]) if d.size else m)
    sides = [Side("a", a), Side("ref", ref, any_align=True)]

    def call(off):
        d_first, d_an = i64(nb, fill=-1), i64(an)
        rc, errs = batch_call(shafa, nb, max(lens), lambda bt, st: bt.compare_dev(st, arena.buf, off["a"], an, d_an, arena.buf,
                                                                                   off["ref"], lens, d_first))
        return dict(rc=rc, errs=errs, first=[int(x) for x in host(d_first)])

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb and res["first"] == want, (label, res["first"], want)

    drive(arena, sides, call, check)


def test_crc32_dev(arena, shafa):
    rng = np.random.default_rng(32)
    lens = [0, 1, 15, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 256 * TILE + 1]
    blocks = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    nb = len(lens)
    want = [zlib.crc32(b.tobytes()) for b in blocks]
    sides = [Side("in", blocks, any_align=True)]

    def call(off):
        import torch
        d_crc, d_n = torch.full((nb,), 0x5A5A5A5A, dtype=torch.int32, device=DEV), i64(lens)
        rc, errs = batch_call(shafa, nb, max(lens), lambda bt, st: bt.crc32_dev(st, arena.buf, off["in"], lens, d_n, d_crc))
        return dict(rc=rc, errs=errs, crc=[int(x) & 0xFFFFFFFF for x in host(d_crc)])

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb and res["crc"] == want, (label, res["crc"], want)

    drive(arena, sides, call, check)


@pytest.mark.parametrize("max_hits", [65536, 5])
def test_find_dev(arena, shafa, max_hits):
    rng = np.random.default_rng(33)
    pat = b"ABC"
    lens = [0, 1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 33]
    blocks = []
    for n in lens:
        b = rng.integers(0x61, 0x7B, n, dtype=np.uint8)                    # no byte of the pattern
        for at in (0, 31, 2047, TILE - 2, TILE, 2 * TILE - 1, n - 3):      # across lane, wave and tile borders, and at the end
            if 0 <= at and at + 3 <= n:
                b[at:at + 3] = np.frombuffer(pat, np.uint8)
        blocks.append(b)
    nb = len(lens)
    pos = [1000000 * (b + 1) for b in range(nb)]
    hits, counts = [], []
    for b, blk in enumerate(blocks):
        raw, at, c = blk.tobytes(), 0, 0
        while (at := raw.find(pat, at)) >= 0:
            hits.append(pos[b] + at)
            at += 1
            c += 1
        counts.append(c)
    assert len(hits) > 5
    sides = [Side("in", blocks, any_align=True)]

    def call(off):
        d_hits, d_count, d_total, d_n = i64(max_hits, fill=-7), i64(nb, fill=-1), i64([0]), i64(lens)
        rc, errs = batch_call(shafa, nb, max(lens), lambda bt, st: bt.find_dev(st, arena.buf, off["in"], lens, d_n, None, pos, pat,
                                                                                max_hits, d_hits, d_count, d_total))
        return dict(rc=rc, errs=errs, hits=[int(x) for x in host(d_hits)], count=[int(x) for x in host(d_count)], total=int(host(d_total)[0]))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        assert res["count"] == counts and res["total"] == len(hits), (label, res["count"], counts)
        k = min(max_hits, len(hits))
        assert res["hits"][:k] == hits[:k] and all(h == -7 for h in res["hits"][k:]), label

    drive(arena, sides, call, check)


# ---------------------------------------------------------------- transposes
def counts_of(T):
    return [0, 1, T - 1, T, T + 1, 3 * T + 5]


def planes_family(arena, shafa, split, merge, k, raws, planes, extra=(), el_any=True, args=()):
    """split(bt, st, *args, el, el_off, ..., planes, plane_off) and merge the other way over blocks whose element bytes are
    `raws` and whose numpy planes are `planes` ([k, n] each); `extra`: further input sides given to both as (tensor, offsets)
    behind the element side"""
    nb = len(raws)
    ns = [len(r) // k for r in raws]
    cap = [n + 5 for n in ns]
    el = [np.frombuffer(r, np.uint8) for r in raws]
    pl = [np.ascontiguousarray(p[j]) for p in planes for j in range(k)]
    more = lambda off: [x for s in extra for x in (arena.buf, off[s.name])]

    def split_call(off):
        d_n = i64(ns)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: getattr(bt, split)(st, k, *args, arena.buf, off["el"], *more(off), cap,
                                                                                   d_n, arena.buf, off["planes"]))
        return dict(rc=rc, errs=errs)

    def split_check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for i, p in enumerate(pl):
            assert res["out"]["planes"][i].tobytes() == p.tobytes(), f"{label}: plane {i % k} of block {i // k}"

    drive(arena, [Side("el", el, any_align=el_any)] + list(extra) + [Side("planes", [p.size for p in pl], out=True, exact=True)],
          split_call, split_check)

    def merge_call(off):
        d_n = i64(ns)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: getattr(bt, merge)(st, k, *args, arena.buf, off["planes"], *more(off),
                                                                                   cap, d_n, arena.buf, off["el"]))
        return dict(rc=rc, errs=errs)

    def merge_check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, r in enumerate(raws):
            assert res["out"]["el"][b].tobytes() == r, f"{label}: elements of block {b}"

    drive(arena, [Side("planes", pl)] + list(extra) + [Side("el", [e.size for e in el], out=True, exact=True, any_align=el_any)],
          merge_call, merge_check)


def transpose(raw, k):
    return np.frombuffer(raw, np.uint8).reshape(-1, k).T


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_planes(arena, shafa, k):
    rng = np.random.default_rng(40 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    planes_family(arena, shafa, "split_planes_dev", "merge_planes_dev", k, raws, [transpose(r, k) for r in raws])


@pytest.mark.parametrize("k", [1, 4])
def test_planes_xor(arena, shafa, k):
    rng = np.random.default_rng(50 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    bases = [rng.integers(0, 256, len(r), dtype=np.uint8) for r in raws]
    planes = [transpose((np.frombuffer(r, np.uint8) ^ b).tobytes(), k) for r, b in zip(raws, bases)]
    planes_family(arena, shafa, "split_planes_xor_dev", "merge_planes_xor_dev", k, raws, planes,
                  extra=[Side("base", bases, any_align=True)])


@pytest.mark.parametrize("k", [1, 4])
def test_planes_diff(arena, shafa, k):
    from test_gpu_planes_grid import _z_planes
    rng = np.random.default_rng(60 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    planes_family(arena, shafa, "split_planes_diff_dev", "merge_planes_diff_dev", k, raws, [_z_planes(r, k, (1,)) for r in raws])


@pytest.mark.parametrize("k", [2, 4])
def test_planes_lag(arena, shafa, k):
    from test_gpu_planes_grid import _z_planes
    rng = np.random.default_rng(70 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    lags = [(1, 3, 17, 4096, 64, 1 << 40)[b] for b in range(len(raws))]
    planes_family(arena, shafa, "split_planes_lag_dev", "merge_planes_lag_dev", k, raws,
                  [_z_planes(r, k, (g,)) for r, g in zip(raws, lags)], el_any=False, args=(lags,))


@pytest.mark.parametrize("k", [1, 4])
def test_planes_grid(arena, shafa, k):
    from test_gpu_planes_grid import _x_bytes, _z_planes
    rng = np.random.default_rng(80 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    lags = [(1, 3), (1, 2), (3, 5, 15), (1, 64, 4096), (1, 17, 153), (16, 4096, 8192)][:len(raws)]
    planes = [_z_planes(r, k, s) for r, s in zip(raws, lags)]
    assert all(_x_bytes(p, k, s) == r for p, s, r in zip(planes, lags, raws))
    planes_family(arena, shafa, "split_planes_grid_dev", "merge_planes_grid_dev", k, raws, planes, el_any=False, args=(lags,))


@pytest.mark.parametrize("w", [3, 17])
def test_records(arena, shafa, w):
    rng = np.random.default_rng(90 + w)
    raws = [rng.integers(0, 256, n * w, dtype=np.uint8).tobytes() for n in counts_of(shafa.PLANES_TILE)]
    nb = len(raws)
    ns = [len(r) // w for r in raws]
    cap = [n + 5 for n in ns]
    rec = [np.frombuffer(r, np.uint8) for r in raws]
    cols = [np.ascontiguousarray(transpose(r, w)[j]) for r in raws for j in range(w)]

    def split_call(off):
        d_n = i64(ns)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: bt.split_records_dev(st, w, arena.buf, off["rec"], cap, d_n, arena.buf,
                                                                                      off["cols"]))
        return dict(rc=rc, errs=errs)

    def split_check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for i, c in enumerate(cols):
            assert res["out"]["cols"][i].tobytes() == c.tobytes(), f"{label}: column {i % w} of block {i // w}"

    drive(arena, [Side("rec", rec, any_align=True), Side("cols", [c.size for c in cols], out=True, exact=True)], split_call, split_check)

    def merge_call(off):
        d_n = i64(ns)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: bt.merge_records_dev(st, w, arena.buf, off["cols"], cap, d_n, arena.buf,
                                                                                      off["rec"]))
        return dict(rc=rc, errs=errs)

    def merge_check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, r in enumerate(raws):
            assert res["out"]["rec"][b].tobytes() == r, f"{label}: records of block {b}"

    drive(arena, [Side("cols", cols), Side("rec", [r.size for r in rec], out=True, exact=True, any_align=True)], merge_call, merge_check)


# ---------------------------------------------------------------- seek index
SPAN = 1024


def seek_case(shafa, oracle):
    """sf_case's 12-bit blocks, their oracle streams and the checkpoints the header defines for a mode-N .shaf: every SPAN
    symbols the bit offset (the sum of the code lengths in front) and the decoded offset k * SPAN"""
    blocks, tables = sf_case(shafa, oracle, "lmax12")
    streams = [oracle.sf_encode(b, t)[1] for b, t in zip(blocks, tables)]
    first, ckpt = [], []
    for b, t in zip(blocks, tables):
        first.append(len(ckpt) // 2)
        bits = np.concatenate([[0], np.cumsum(t.lens()[b].astype(np.int64))])
        for k in range(max(1, -(-b.size // SPAN))):
            ckpt += [int(bits[k * SPAN]), k * SPAN]
    return blocks, tables, streams, first, ckpt


def test_seek_index_dev(arena, shafa, oracle):
    import torch
    blocks, tables, _, first, ckpt = seek_case(shafa, oracle)
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    _, d_tables = table_bytes(shafa, tables)
    sides = [Side("in", blocks)]

    def call(off):
        d_ckpt, d_n, d_sizes = i64(len(ckpt), fill=-1), i64(nb, fill=-1), i64(sizes)
        d_status = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
        rc, errs = batch_call(shafa, nb, max(sizes), lambda bt, st: bt.seek_index_dev(st, arena.buf, off["in"], sizes, d_sizes, d_tables,
                                                                                     SPAN, shafa.SEEK_SF, first, d_ckpt, d_status, d_n))
        return dict(rc=rc, errs=errs, ckpt=[int(x) for x in host(d_ckpt)], status=[int(x) for x in host(d_status)],
                    n=[int(x) for x in host(d_n)])

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb and res["status"] == [0] * nb and res["n"] == sizes, label
        assert res["ckpt"] == ckpt, label

    drive(arena, sides, call, check)


def test_read_spans_dev(arena, shafa, oracle):
    """two ranges a block, read from the payloads where they lie: the whole block, and one from inside a span to inside another"""
    blocks, tables, streams, first, ckpt = seek_case(shafa, oracle)
    nb = len(blocks)
    _, d_tables = table_bytes(shafa, tables)
    ranges = []
    for b, blk in enumerate(blocks):
        ranges.append((b, 0, blk.size))
        if blk.size > 3 * SPAN:
            ranges.append((b, SPAN // 2 + 1, blk.size - SPAN - 7))
    want = [blocks[b][lo:hi] for b, lo, hi in ranges]
    sides = [Side("pay", streams, any_align=True), Side("out", [w.size for w in want], out=True, exact=True)]

    def call(off):
        d_ckpt = i64(ckpt)
        items = [(b, lo // SPAN, (hi - 1) // SPAN, lo, hi, dst) for (b, lo, hi), dst in zip(ranges, off["out"])]
        rc, errs = batch_call(shafa, len(items), 1 << 20, lambda bt, st: bt.read_spans_dev(
            st, arena.buf, off["pay"], [s.size for s in streams], [b.size for b in blocks], first, d_tables, SPAN, shafa.SEEK_SF, d_ckpt,
            items, arena.buf))
        return dict(rc=rc, errs=errs)

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * len(ranges), label
        for i, w in enumerate(want):
            assert res["out"]["out"][i].tobytes() == w.tobytes(), f"{label}: range {ranges[i]}"

    drive(arena, sides, call, check)


# ---------------------------------------------------------------- files in device memory
def payload_file(shafa, framing, blocks):
    """test_gpu_pack._payload_file: a .rle is the payloads back to back, a .shaf "@n" and "@size@payload" per block"""
    if framing == shafa.FRAME_RAW:
        return b"".join(blocks)
    return b"@" + str(len(blocks)).encode() + b"".join(b"@" + str(len(b)).encode() + b"@" + b for b in blocks)


def payloads():
    rng = np.random.default_rng(110)
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 17, TILE - 1, TILE + 1, 3 * TILE + 5)]


@pytest.mark.parametrize("framing", ["FRAME_RAW", "FRAME_SHAF"])
@pytest.mark.parametrize("files", [False, True], ids=["pack_payloads", "pack_payloads_files"])
def test_pack_payloads(arena, shafa, framing, files):
    framing = getattr(shafa, framing)
    blocks = payloads()
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    caps = [n + 7 for n in sizes]
    groups = [(0, 2), (2, 3)] if files else [(0, nb)]
    room = [shafa.pack_payloads_max(caps[a:a + c], framing) for a, c in groups]
    want = [payload_file(shafa, framing, [b.tobytes() for b in blocks[a:a + c]]) for a, c in groups]
    sides = [Side("src", blocks), Side("dst", room, out=True, exact=True, any_align=True)]

    def call(off):
        d_n, d_len = i64(sizes), i64(len(groups), fill=-1)
        if files:
            body = lambda bt, st: bt.pack_payloads_files(st, [a for a, _ in groups], [c for _, c in groups], framing, arena.buf, off["src"],
                                                         caps, d_n, arena.buf, off["dst"], room, d_len)
        else:
            body = lambda bt, st: bt.pack_payloads(st, framing, arena.buf, off["src"], caps, d_n, arena.buf[off["dst"][0]:], room[0], d_len)
        rc, errs = batch_call(shafa, nb, max(caps), body)
        n = [int(x) for x in host(d_len)]
        return dict(rc=rc, errs=errs, n=n, used={"dst": [min(max(x, 0), r) for x, r in zip(n, room)]})

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for f, w in enumerate(want):
            assert res["n"][f] == len(w) and res["out"]["dst"][f][:len(w)].tobytes() == w, f"{label}: file {f}"
            assert bool((res["out"]["dst"][f][len(w):] == FILL).all()), f"{label}: bytes behind file {f}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("kind", ["cod", "freq"])
@pytest.mark.parametrize("files", [False, True], ids=["pack", "pack_files"])
def test_pack_texts(arena, shafa, oracle, kind, files):
    """pack_cod / pack_freq and their _files forms: the destination is the side with offsets; the expected text is the host
    formatter's (test_gpu_pack._text_file)"""
    import torch
    blocks = [zipf(shafa, oracle, 120 + i, n) for i, n in enumerate((700, 3000, 70000))]
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    freqs = [oracle.hist256(b) for b in blocks]
    tarr, d_tables = table_bytes(shafa, [oracle.sf_build(f) for f in freqs])
    texts = [shafa.cod_format(tarr[i]) if kind == "cod" else shafa.freq_format(f) for i, f in enumerate(freqs)]
    groups = [(0, 1), (1, 2)] if files else [(0, nb)]
    modes = [b"R", b"N"][:len(groups)]

    def text_file(mode, a, c):
        out = b"@" + mode + b"@" + str(c).encode()
        for n, t in zip(sizes[a:a + c], texts[a:a + c]):
            out += b"@" + str(n).encode() + b"@" + bytes(t)
        return out + b"@0"

    want = [text_file(m, a, c) for m, (a, c) in zip(modes, groups)]
    room = [(shafa.pack_cod_max if kind == "cod" else shafa.pack_freq_max)(c) for _, c in groups]
    d_freq = torch.from_numpy(np.concatenate(freqs).astype(np.int64)).to(DEV)
    d_body = d_tables if kind == "cod" else d_freq
    sides = [Side("dst", room, out=True, exact=True, any_align=True)]

    def call(off):
        d_sizes, d_len = i64(sizes), i64(len(groups), fill=-1)
        if files:
            body = lambda bt, st: getattr(bt, f"pack_{kind}_files")(st, [a for a, _ in groups], [c for _, c in groups], modes, d_sizes,
                                                                    d_body, arena.buf, off["dst"], room, d_len)
        else:
            body = lambda bt, st: getattr(bt, f"pack_{kind}")(st, nb, modes[0], d_sizes, d_body, arena.buf[off["dst"][0]:], room[0], d_len)
        rc, errs = batch_call(shafa, nb, 1 << 20, body)
        n = [int(x) for x in host(d_len)]
        return dict(rc=rc, errs=errs, n=n, used={"dst": [min(max(x, 0), r) for x, r in zip(n, room)]})

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for f, w in enumerate(want):
            assert res["n"][f] == len(w) and res["out"]["dst"][f][:len(w)].tobytes() == w, f"{label}: file {f}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("kind", ["payloads", "cod", "freq"])
def test_pack_files_one_file_short_of_room(arena, shafa, oracle, kind):
    """three files of one block each, the middle one with a region one byte shorter than the file: LACK_OF_MEMORY on its first
    block, the length it needs in d_dst_n, no byte of its region written; the files around it written normally"""
    import torch
    blocks = [zipf(shafa, oracle, 140 + i, n) for i, n in enumerate((700, TILE + 1, 3000))]
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    if kind == "payloads":
        want = [payload_file(shafa, shafa.FRAME_SHAF, [b.tobytes()]) for b in blocks]
        sides = [Side("src", blocks)]
    else:
        freqs = [oracle.hist256(b) for b in blocks]
        tarr, d_tables = table_bytes(shafa, [oracle.sf_build(f) for f in freqs])
        texts = [shafa.cod_format(tarr[i]) if kind == "cod" else shafa.freq_format(f) for i, f in enumerate(freqs)]
        want = [b"@N@1@" + str(n).encode() + b"@" + bytes(t) + b"@0" for n, t in zip(sizes, texts)]
        d_body = d_tables if kind == "cod" else torch.from_numpy(np.concatenate(freqs).astype(np.int64)).to(DEV)
        sides = []
    room = [len(w) + 9 for w in want]
    room[1] = len(want[1]) - 1
    sides.append(Side("dst", room, out=True, exact=True, any_align=True))
    first, count = list(range(nb)), [1] * nb

    def call(off):
        d_n, d_len = i64(sizes), i64(nb, fill=-1)
        if kind == "payloads":
            body = lambda bt, st: bt.pack_payloads_files(st, first, count, shafa.FRAME_SHAF, arena.buf, off["src"], sizes, d_n, arena.buf,
                                                         off["dst"], room, d_len)
        else:
            body = lambda bt, st: getattr(bt, f"pack_{kind}_files")(st, first, count, [b"N"] * nb, d_n, d_body, arena.buf, off["dst"], room,
                                                                    d_len)
        rc, errs = batch_call(shafa, nb, 1 << 20, body)
        return dict(rc=rc, errs=errs, n=[int(x) for x in host(d_len)])

    def check(res, label):
        assert res["rc"] == shafa.LACK_OF_MEMORY and res["errs"] == [0, shafa.LACK_OF_MEMORY, 0], (label, res["errs"])
        assert res["n"] == [len(w) for w in want], (label, res["n"])
        for f, w in enumerate(want):
            got = res["out"]["dst"][f]
            if f == 1:
                assert bool((got == FILL).all()), f"{label}: the refused file left bytes in its region"
            else:
                assert got[:len(w)].tobytes() == w and bool((got[len(w):] == FILL).all()), f"{label}: file {f}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("kind,files", [("cod", False), ("cod", True), ("freq", False), ("rle_freq", False), ("rle_freq", True)],
                         ids=["unpack_cod", "unpack_cod_files", "unpack_freq", "unpack_rle_freq", "unpack_rle_freq_files"])
def test_unpack_texts(arena, shafa, oracle, kind, files):
    """unpack_cod, unpack_freq, unpack_rle_freq and the _files forms (the text at the arena's base + a far offset) over the host
    formatter's texts: the tables, counts, sizes and payload places that went into the text come back"""
    import ctypes as C
    import torch
    blocks = [zipf(shafa, oracle, 130 + i, n) for i, n in enumerate((700, 3000, 70000))]
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    freqs = [oracle.hist256(b) for b in blocks]
    tarr, _ = table_bytes(shafa, [oracle.sf_build(f) for f in freqs])
    texts = [shafa.cod_format(tarr[i]) if kind == "cod" else shafa.freq_format(f) for i, f in enumerate(freqs)]
    text = b"@R@" + str(nb).encode() + b"".join(b"@" + str(n).encode() + b"@" + bytes(t) for n, t in zip(sizes, texts)) + b"@0"
    tsz = C.sizeof(shafa.CodeTable)
    sides = [Side("text", [np.frombuffer(text, np.uint8)], any_align=True)]

    def call(off):
        at = off["text"][0]
        view = arena.buf[at:at + len(text)]
        base = arena.buf.data_ptr()
        d_info = torch.full((shafa.UNPACK_INFO_WORDS,), -1, dtype=torch.int64, device=DEV)
        d_a, d_b = i64(nb, fill=-1), i64(nb, fill=-1)
        d_tab = torch.full((nb * tsz,), 0xA5, dtype=torch.uint8, device=DEV)
        d_cnt = i64(nb * 256, fill=-1)

        def body(bt, st):
            if kind == "cod":
                bt.unpack_cod_files(st, [0], [nb], base, [at], [len(text)], d_info, d_a, d_tab) if files else \
                    bt.unpack_cod(st, nb, view, d_info, d_a, d_tab)
            elif kind == "freq":
                bt.unpack_freq(st, nb, view, d_info, d_a, d_cnt)
            else:
                bt.unpack_rle_freq_files(st, [0], [nb], base, [at], [len(text)], [0], [sum(sizes)], d_info, d_a, d_b) if files else \
                    bt.unpack_rle_freq(st, nb, view, sum(sizes), d_info, d_a, d_b)
        rc, errs = batch_call(shafa, nb, 1 << 20, body)
        return dict(rc=rc, errs=errs, info=host(d_info), a=[int(x) for x in host(d_a)], b=[int(x) for x in host(d_b)], tab=host(d_tab),
                    cnt=host(d_cnt).reshape(nb, 256))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        if kind == "cod":
            assert res["a"] == sizes and res["tab"].tobytes() == bytes(tarr), label
        elif kind == "freq":
            assert res["a"] == sizes and np.array_equal(res["cnt"].astype(np.uint64), np.stack(freqs)), label
        else:
            assert res["a"] == [sum(sizes[:b]) for b in range(nb)] and res["b"] == sizes, label

    drive(arena, sides, call, check)


@pytest.mark.parametrize("entry", ["unpack_payloads", "unpack_payloads_at", "unpack_shaf_files"])
def test_unpack_shaf_and_payloads(arena, shafa, entry):
    """a .shaf file of five payloads: unpack_shaf gives each payload's place, unpack_payloads moves them to 16-aligned regions;
    through unpack_shaf_files and unpack_payloads_at the places are measured from the arena's base, so a far file's are past 2^32"""
    unpack_family(arena, shafa, entry)


@pytest.mark.parametrize("entry", ["unpack_payloads", "unpack_payloads_at"])
def test_unpack_payloads_one_region_short_of_room(arena, shafa, entry):
    """payload 3 (8193 bytes) has a region of 8192: OUTSIDE_MODULE for it alone and no byte of its region written, the other
    payloads whole"""
    unpack_family(arena, shafa, entry, short=3)


def unpack_family(arena, shafa, entry, short=None):
    import torch
    blocks = payloads()
    nb = len(blocks)
    text = payload_file(shafa, shafa.FRAME_SHAF, [b.tobytes() for b in blocks])
    places, pos = [], len(b"@" + str(nb).encode())
    for b in blocks:
        pos += len(b"@" + str(b.size).encode() + b"@")
        places.append(pos)
        pos += b.size
    assert pos == len(text)
    sizes = [b.size for b in blocks]
    caps = [al16(n) for n in sizes]
    if short is not None:
        caps[short] -= 16
        assert caps[short] < sizes[short]
    expect = {} if short is None else {short: shafa.OUTSIDE_MODULE}
    sides = [Side("file", [np.frombuffer(text, np.uint8)], any_align=True), Side("dst", caps, out=True)]

    def call(off):
        at = off["file"][0]
        view = arena.buf[at:at + len(text)]
        d_count = torch.zeros(8, dtype=torch.int64, device=DEV)
        d_count[0] = nb
        d_off, d_n = i64(nb, fill=-1), i64(nb, fill=-1)

        def body(bt, st):
            if entry == "unpack_shaf_files":
                bt.unpack_shaf_files(st, [0], [nb], arena.buf.data_ptr(), [at], [len(text)], d_count, d_off, d_n)
                bt.unpack_payloads_at(st, arena.buf.data_ptr(), at + len(text), d_off, d_n, arena.buf, off["dst"], caps)
            else:
                bt.unpack_shaf(st, nb, view, d_count, d_off, d_n)
                if entry == "unpack_payloads_at":
                    bt.unpack_payloads_at(st, view.data_ptr(), len(text), d_off, d_n, arena.buf, off["dst"], caps)
                else:
                    bt.unpack_payloads(st, view, d_off, d_n, arena.buf, off["dst"], caps)
        rc, errs = batch_call(shafa, nb, max(caps), body)
        base = at if entry == "unpack_shaf_files" else 0
        return dict(rc=rc, errs=errs, places=[int(x) - base for x in host(d_off)], n=[int(x) for x in host(d_n)],
                    used={"dst": [min(n, c) for n, c in zip(sizes, caps)]})

    def check(res, label):
        assert (res["rc"] == 0) == (not expect) and res["errs"] == [expect.get(b, 0) for b in range(nb)], (label, res["errs"])
        assert res["places"] == places and res["n"] == sizes, (label, res["places"], places)
        for b, blk in enumerate(blocks):
            if b in expect:
                assert bool((res["out"]["dst"][b] == FILL).all()), f"{label}: the refused payload {b} left bytes in its region"
            else:
                assert res["out"]["dst"][b][:blk.size].tobytes() == blk.tobytes(), f"{label}: payload {b}"

    drive(arena, sides, call, check)


# ---------------------------------------------------------------- quantised and rounded fields
def field_case(shafa, kind, k):
    """four blocks of test_gpu_fields' (quant) or test_gpu_rounding's (round) values with their models: the codes' planes
    (test_gpu_planes_grid._z_planes), what the merge leaves, the sorted outlier records and the planes' histograms"""
    import test_gpu_fields as fld
    import test_gpu_rounding as rnd
    from test_gpu_planes_grid import _z_planes
    T = shafa.PLANES_TILE
    counts = (1, T - 1, T + 1, 2 * T + 3)
    rows = [(1,), (1, 3), (2, 3, 5), (1, 16, T)]
    c = dict(ns=list(counts), lags=rows, A=[], B=[], x=[], planes=[], restored=[], rec=[])
    for b, n in enumerate(counts):
        if kind == "quant":
            step = (2.0 ** -10, fld._exact(1e-3, k), fld._exact(0.37, k), 3.0)[b]
            bound = fld._exact(step * (0.5 + 2.0 ** -6), k)
            x = fld._values(n, k, step, T, 10 * k + b)
            code, xr, good = fld._model(x, step, bound)
            back, rec = fld._restored(x, xr, good), fld._records(x, good)
            c["A"].append(step), c["B"].append(bound)
        else:
            fmt = {2: ("bfloat16", "float16"), 4: ("float32",), 8: ("float64",)}[k][b % (2 if k == 2 else 1)]
            keep = (2, rnd.MANT[fmt] // 2, 0, rnd.MANT[fmt])[b]
            x = rnd._values(n, fmt, keep, T, 10 * k + b)
            code, xr, good = rnd._rule(x, rnd.MANT[fmt], keep)
            back, rec = rnd._restored(x, xr, good), rnd._records(x, good)
            c["A"].append(rnd.MANT[fmt]), c["B"].append(keep)
        c["x"].append(np.ascontiguousarray(x).view(np.uint8))
        c["planes"].append(_z_planes(code.tobytes(), k, rows[b]))
        c["restored"].append(np.ascontiguousarray(back).view(np.uint8))
        c["rec"].append(np.ascontiguousarray(rec, dtype=np.uint64))
    assert sum(len(r) for r in c["rec"]) > 10
    c["freq"] = np.stack([np.stack([np.bincount(p[j], minlength=256) for j in range(k)]) for p in c["planes"]]).astype(np.int64)
    return c


FIELDS = [("quant", 4), ("quant", 8), ("round", 2), ("round", 4), ("round", 8)]


@pytest.mark.parametrize("kind,k", FIELDS)
def test_field_split(arena, shafa, kind, k):
    c = field_case(shafa, kind, k)
    nb, ns = len(c["ns"]), c["ns"]
    pl = [np.ascontiguousarray(p[j]) for p in c["planes"] for j in range(k)]
    roff = [sum(ns[:b]) for b in range(nb)]                                # room for every element of a block, in records
    sides = [Side("el", c["x"]), Side("planes", [p.size for p in pl], out=True, exact=True),
             Side("outl", [16 * sum(ns)], out=True, exact=True)]

    def call(off):
        d_n, d_cnt = i64(ns), i64(nb, fill=-1)
        at = off["outl"][0]
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: getattr(bt, f"split_planes_grid_{kind}_dev")(
            st, k, c["lags"], c["A"], c["B"], arena.buf, off["el"], ns, d_n, arena.buf, off["planes"], arena.buf.data_ptr() + at, roff, ns,
            d_cnt))
        cnt = [int(x) for x in host(d_cnt)]
        img = host(arena.buf[at:at + 16 * sum(ns)]).view(np.uint64).reshape(-1, 2)
        rec = [img[o:o + min(max(m, 0), n)] for o, m, n in zip(roff, cnt, ns)]
        rec = [r[np.argsort(r[:, 0], kind="stable")] for r in rec]         # a block's records come in any order
        return dict(rc=rc, errs=errs, cnt=cnt, rec=rec, used={"outl": [0]})

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for i, p in enumerate(pl):
            assert res["out"]["planes"][i].tobytes() == p.tobytes(), f"{label}: plane {i % k} of block {i // k}"
        assert res["cnt"] == [len(r) for r in c["rec"]], label
        for b, r in enumerate(c["rec"]):
            assert res["rec"][b].tobytes() == r.tobytes(), f"{label}: outlier records of block {b}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("kind,k", FIELDS)
def test_field_merge(arena, shafa, kind, k):
    c = field_case(shafa, kind, k)
    nb, ns = len(c["ns"]), c["ns"]
    pl = [np.ascontiguousarray(p[j]) for p in c["planes"] for j in range(k)]
    found = [len(r) for r in c["rec"]]
    roff = [sum(found[:b]) for b in range(nb)]
    recs = np.concatenate(c["rec"]).reshape(-1).view(np.uint8)
    par = (c["A"],) if kind == "quant" else (c["A"], c["B"])
    sides = [Side("planes", pl), Side("outl", [recs]), Side("el", [x.size for x in c["x"]], out=True, exact=True)]

    def call(off):
        d_n = i64(ns)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: getattr(bt, f"merge_planes_grid_{kind}_dev")(
            st, k, c["lags"], *par, arena.buf, off["planes"], ns, d_n, arena.buf.data_ptr() + off["outl"][0], roff, found, arena.buf,
            off["el"]))
        return dict(rc=rc, errs=errs)

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, w in enumerate(c["restored"]):
            assert res["out"]["el"][b].tobytes() == w.tobytes(), f"{label}: elements of block {b}"

    drive(arena, sides, call, check)


@pytest.mark.parametrize("kind,k", FIELDS)
def test_field_hist(arena, shafa, kind, k):
    c = field_case(shafa, kind, k)
    nb, ns = len(c["ns"]), c["ns"]
    sides = [Side("in", c["x"])]

    def call(off):
        d_n, d_cnt, d_freq = i64(ns), i64(nb, fill=-1), i64(nb * k * 256, fill=-1)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: getattr(bt, f"hist_planes_grid_{kind}_dev")(
            st, k, c["lags"], c["A"], c["B"], arena.buf, off["in"], ns, d_n, d_freq, d_cnt))
        return dict(rc=rc, errs=errs, cnt=[int(x) for x in host(d_cnt)], freq=host(d_freq).reshape(nb, k, 256))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        assert res["cnt"] == [len(r) for r in c["rec"]] and np.array_equal(res["freq"], c["freq"]), label

    drive(arena, sides, call, check)


def _error_entries():
    import test_gpu_grid_walks as gw
    return gw.ENTRIES


@pytest.mark.parametrize("entry,k", [(e, k) for e in ("pair", "quant", "round") for k in ((2, 4, 8) if e != "quant" else (4, 8))])
def test_error_entries(arena, shafa, entry, k):
    """error_dev ("pair": what came back, a, against the original, x), error_quant_dev and error_round_dev over
    test_gpu_grid_walks.error_run_blocks, all twelve words against its exact_record"""
    import test_gpu_grid_walks as gw
    import test_gpu_quality as q
    assert (entry, k) in _error_entries()
    T = shafa.PLANES_TILE
    blks = gw.error_run_blocks(shafa, entry, k)
    want = [gw._want(entry, b, T)[1] for b in blks]
    nb = len(blks)
    ns = [b["x"].size for b in blks]
    sides = [Side("x", [np.ascontiguousarray(b["x"]).view(np.uint8) for b in blks])]
    if entry == "pair":
        sides.append(Side("a", [np.ascontiguousarray(b["y"]).view(np.uint8) for b in blks]))

    def call(off):
        d_stat, d_n = i64(q.W12 * nb, fill=-1), i64(ns)
        if entry == "round":
            body = lambda bt, st: bt.error_round_dev(st, k, [q.MANT[b["fmt"]] for b in blks], [b["keep"] for b in blks], arena.buf,
                                                     off["x"], ns, d_n, d_stat)
        elif entry == "quant":
            body = lambda bt, st: bt.error_quant_dev(st, k, [b["step"] for b in blks], [b["bound"] for b in blks], arena.buf, off["x"],
                                                     ns, d_n, d_stat)
        else:
            body = lambda bt, st: bt.error_dev(st, k, [q.MANT[b["fmt"]] for b in blks], [b["abs"] for b in blks],
                                               [b["rel"] for b in blks], arena.buf, off["a"], ns, d_n, arena.buf, off["x"], d_stat)
        rc, errs = batch_call(shafa, nb, 1 << 20, body)
        return dict(rc=rc, errs=errs, stat=host(d_stat).view(np.uint64).reshape(nb, q.W12))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        for b, ex in enumerate(want):
            got = [int(v) for v in res["stat"][b]]
            assert got == ex, (label, b, [i for i in range(q.W12) if got[i] != ex[i]])

    drive(arena, sides, call, check)


@pytest.mark.parametrize("k", [2, 4])
def test_hist_planes_grid_dev(arena, shafa, k):
    from test_planes_grid_hist_cpu import plane_histograms
    U = {2: np.uint16, 4: np.uint32}[k]
    rng = np.random.default_rng(100 + k)
    raws = [rng.integers(0, 256, n * k, dtype=np.uint8) for n in counts_of(shafa.PLANES_TILE)]
    lags = [(1, 3), (), (3, 5, 15), (1, 64, 4096), (1,), (16, 4096, 8192)][:len(raws)]
    nb = len(raws)
    ns = [r.size // k for r in raws]
    want = np.stack([plane_histograms(r.view(U), s) for r, s in zip(raws, lags)]).astype(np.int64)
    sides = [Side("in", raws)]

    def call(off):
        d_n, d_freq = i64(ns), i64(nb * k * 256, fill=-1)
        rc, errs = batch_call(shafa, nb, 1 << 20, lambda bt, st: bt.hist_planes_grid_dev(st, k, lags, arena.buf, off["in"], ns, d_n, d_freq))
        return dict(rc=rc, errs=errs, freq=host(d_freq).reshape(nb, k, 256))

    def check(res, label):
        assert res["rc"] == 0 and res["errs"] == [0] * nb, label
        assert np.array_equal(res["freq"], want), label

    drive(arena, sides, call, check)
