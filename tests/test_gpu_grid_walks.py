"""The walks of csrc/planes_lag.hip where the families' own files never took them, against numpy on the host; nothing is compared
with device code.

A. Runs of tiles per workgroup.  tile_setup gives a workgroup ceil(tiles / 16384) consecutive tiles of the call, counted from the
   capacities.  Capacities [3 T + 5, 2^28, 20000] make 32775 tiles and three tiles a workgroup; workgroup 1 walks the last tile of
   block 0 (5 elements) and the first two of block 1, so whatever a block owns (lags, step and bound, format and keep, record
   place, plane offsets, ref_off, the alignment switch) changes inside one run, and planes_error_tiles' two LDS halves take a
   second and a third turn.  The 2^28 capacity costs tile bookkeeping only: the sizes are small.
B. Blocks of 256, 257 and 514 tiles through planes_error_blocks: a thread folds per = 1, 2 and 3 partials.
C. The fold order of "Error statistics" (include/shafa_hip.h), bit for bit: exact_sum is the header's order in float64, one numpy
   operation one IEEE operation, and all twelve words are compared for equality; the fsum tolerance of test_gpu_quality stays
   beside it as a check of the model.  tests/test_grid_walks_cpu.py shows that the comparison is not vacuous.
D. The alignments of the families merged after test_gpu_every_alignment_lag.py: the rounding split, merge and histogram and the
   quantised histogram over tables of that file's kind (every own alignment, every (own, tap) pair, every zeroed-head byte count,
   every last-unit count, the restore pass's cut words at every (start, end) mod 16), and the error entries with the x side at
   every multiple of the element size below 16, crossed with the counts 1 .. 17 and T +- 1.

The references, the 0xA5 images compared whole and the guards are the families' own (test_gpu_quality._record / _round / _quant /
_values / _Image / _came_back, test_gpu_planes_grid._Layout, test_gpu_fields._model / _Layout, test_gpu_rounding._Layout) and the
class assertions over the real device addresses are test_gpu_every_alignment_lag.py's.  One launch per direction, family and
element size.  The tables are plain functions of the tile size, so the CPU file checks them without a GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_every_alignment_lag as eal
import test_gpu_fields as fld
import test_gpu_planes_grid as grd
import test_gpu_planes_lag as lag
import test_gpu_quality as q
import test_gpu_rounding as rnd
from test_gpu_every_alignment import _once

pytestmark = pytest.mark.gpu

TILE_WGS = 16384                                                           # workgroups of a tiles kernel: ceil(tiles / TILE_WGS) tiles each
THREADS, UNIT, WAVE = 256, 16, 64                                          # a workgroup's threads, a lane's elements a unit, a wave's lanes
BIG_CAP = 1 << 28
ERR_ELEMS = {"pair": (2, 4, 8), "quant": (4, 8), "round": (2, 4, 8)}
ENTRIES = [(e, k) for e in ("pair", "quant", "round") for k in ERR_ELEMS[e]]
A_OFF = {1: (1, 2, 7), 2: (1, 2, 5), 4: (1, 2, 3), 8: (1, 0, 1)}            # elements behind a multiple of 64 bytes, a block each
INF_BITS = q._b(math.inf)


# ---------------------------------------------------------------- C. the header's order of the two sums
def _tree(a):
    """[..., 64] -> [...]: for d = 1, 2, .. 32 lane l < 64 - d takes a[l] + a[l + d], all lanes at once; lane 0 ends with the wave's"""
    a = a.copy()
    d = 1
    while d < WAVE:
        a[..., :WAVE - d] = a[..., :WAVE - d] + a[..., d:]
        d <<= 1
    return a[..., 0]


def _waves(w):
    """[..., 4] -> [...]: ((w0 + w1) + w2) + w3"""
    r = w[..., 0]
    for j in range(1, w.shape[-1]):
        r = r + w[..., j]
    return r


def lane_sums(term, fin, T):
    """[tiles, THREADS]: a lane's terms of a tile in the order u = 0, 1 .., i = 0 .. 15 over the elements u * 4096 + lane * 16 + i,
    from +0.0; an element that is not finite or past the end adds nothing"""
    n = term.size
    nt = -(-n // T)
    units = T // (THREADS * UNIT)
    assert units * THREADS * UNIT == T
    x, m = np.zeros(nt * T), np.zeros(nt * T, bool)
    x[:n], m[:n] = np.where(fin, term, 0.0), fin
    x, m = x.reshape(nt, units, THREADS, UNIT), m.reshape(nt, units, THREADS, UNIT)
    acc = np.zeros((nt, THREADS))
    for u in range(units):
        for i in range(UNIT):
            acc = np.where(m[:, u, :, i], acc + x[:, u, :, i], acc)
    return acc


def tile_partials(term, fin, T):
    """one partial a tile: the tree across each wave, the waves in order"""
    return _waves(_tree(lane_sums(term, fin, T).reshape(-1, THREADS // WAVE, WAVE)))


def block_fold(part):
    """planes_error_blocks: thread j adds its per = ceil(tiles / 256) consecutive partials to +0.0 in order, then the same tree"""
    nt = part.size
    per = -(-nt // THREADS)
    p = np.zeros(per * THREADS)
    p[:nt] = part
    p = p.reshape(THREADS, per)
    acc = np.zeros(THREADS)
    for j in range(per):
        acc = acc + p[:, j]
    return float(_waves(_tree(acc.reshape(THREADS // WAVE, WAVE))))


def exact_sum(term, fin, T):
    """the sum of term over fin as the header orders it: every + one IEEE double addition"""
    if term.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return block_fold(tile_partials(term, fin, T))


def exact_record(xb, yb, fmt, T, outliers=0, abs_b=None, rel_b=0.0):
    """(test_gpu_quality._record's words with the fsum sums as floats, the twelve words as the device must give them bit for
    bit).  The model is checked against fsum here, within the bound test_gpu_quality._same gives the device."""
    with np.errstate(over="ignore"):                                       # x x may overflow: carried as IEEE carries it
        w = q._record(xb, yb, fmt, outliers, abs_b, rel_b)
    x, y = q._dbl(xb, fmt), q._dbl(yb, fmt)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(all="ignore"):
        e = np.abs(x - y)
        sums = [exact_sum(e * e, fin, T), exact_sum(x * x, fin, T)]
    for s, f in zip(sums, w[6:8]):
        if math.isfinite(f):
            assert abs(s - f) <= max(xb.size, 1) * 2.0 ** -52 * f, (s, f)
        else:
            assert s == f == math.inf
    ex = list(w)
    ex[6], ex[7] = q._b(sums[0]), q._b(sums[1])
    return w, ex


# ---------------------------------------------------------------- one launch of an error entry
def _want(entry, b, T):
    if "want" not in b:
        x, fmt = b["x"], b["fmt"]
        if entry == "pair":
            b["want"] = exact_record(x, b["y"], fmt, T, 0, b["abs"], b["rel"])
        else:
            y, good = q._round(x, q.MANT[fmt], b["keep"]) if entry == "round" else q._quant(x, b["step"], b["bound"])
            b["want"] = exact_record(x, y, fmt, T, int((~good).sum()))
    return b["want"]


def _launch(shafa, entry, k, blks, caps=None, classes=None):
    """blks: dicts of name, x (bits), fmt, a (the x side's elements behind a multiple of 64 bytes) and keep | step, bound | y, abs,
    rel.  The whole d_stat, guard words included, against exact_record; the inputs come back unchanged."""
    T = shafa.PLANES_TILE
    nb = len(blks)
    xs = [b["x"] for b in blks]
    ns = [x.size for x in xs]
    caps = ns if caps is None else caps
    wants = [_want(entry, b, T) for b in blks]
    R = q._Image(k, xs, [b["a"] for b in blks])
    st = q._stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_x, d_stat, d_n = q._to(R.img), q._fill64(q.W12 * nb + 2), q._sizes(ns)
        addr = [d_x.data_ptr() + o for o in R.off]
        assert [p % 16 for p in addr] == [b["a"] * k % 16 for b in blks]
        if classes is not None:
            classes(addr)
        if entry == "round":
            bt.error_round_dev(st, k, [q.MANT[b["fmt"]] for b in blks], [b["keep"] for b in blks], d_x, R.off, caps, d_n, d_stat[1:-1])
        elif entry == "quant":
            bt.error_quant_dev(st, k, [b["step"] for b in blks], [b["bound"] for b in blks], d_x, R.off, caps, d_n, d_stat[1:-1])
        else:
            A = q._Image(k, [b["y"] for b in blks], [0] * nb)
            d_a = q._to(A.img)
            assert d_a.data_ptr() % 16 == 0 and not any(o % 16 for o in A.off)
            bt.error_dev(st, k, [q.MANT[b["fmt"]] for b in blks], [b["abs"] for b in blks], [b["rel"] for b in blks], d_a, A.off, caps,
                         d_n, d_x, R.off, d_stat[1:-1])
        assert bt.finish(st, nb) == (0, [0] * nb), (entry, k)
        got = d_stat.cpu().numpy().view(np.uint64)
        assert got.size == q.W12 * nb + 2 and got[0] == q.FILL64 and got[-1] == q.FILL64, (entry, k)
        for b, (fs, ex) in enumerate(wants):
            g = [int(v) for v in got[1 + q.W12 * b:1 + q.W12 * (b + 1)]]
            what = (entry, k, b, blks[b]["name"])
            if math.isfinite(fs[6]) and math.isfinite(fs[7]):
                q._same(g, fs, what)
            assert g == ex, (what, "words that differ", [i for i in range(q.W12) if g[i] != ex[i]], g, ex)
        assert d_x.cpu().numpy().tobytes() == R.img.tobytes(), (entry, k)
        if entry == "pair":
            assert d_a.cpu().numpy().tobytes() == A.img.tobytes(), k
    finally:
        bt.close()


def came_back(x, fmt, seed):
    """test_gpu_quality._came_back, and every third finite pair rounded four bits shorter: at float64 e then has more than 26
    bits, so e e rounds and a contracted se2 + e e shows (test_grid_walks_cpu.py)"""
    y = q._came_back(x, fmt, seed).copy()
    SIGN, INF, _ = q._consts(fmt)
    U = x.dtype.type
    both = np.flatnonzero(((x & U(SIGN - 1)) < U(INF)) & ((y & U(SIGN - 1)) < U(INF)))[::3]
    y[both] = q._round(x, q.MANT[fmt], max(q.MANT[fmt] // 2 - 4, 0))[0][both]
    return y


# ---------------------------------------------------------------- A. runs of tiles per workgroup
def run_caps(T):
    return [3 * T + 5, BIG_CAP, 20000]


def run_of(w, caps, T):
    """(block, tile of the block) of every tile workgroup w walks"""
    tiles = [-(-c // T) for c in caps]
    per_wg = -(-sum(tiles) // TILE_WGS)
    out = []
    for g in range(w * per_wg, min((w + 1) * per_wg, sum(tiles))):
        b = 0
        while g >= tiles[b]:
            g -= tiles[b]
            b += 1
        out.append((b, g))
    return out


def assert_runs(T, ns):
    """three tiles a workgroup; workgroup 1 ends block 0 with a tile of 5 elements and starts block 1, with data on both sides"""
    caps = run_caps(T)
    tiles = [-(-c // T) for c in caps]
    assert tiles == [4, 32768, 3] and sum(tiles) == 32775 and -(-sum(tiles) // TILE_WGS) == 3
    assert run_of(0, caps, T) == [(0, 0), (0, 1), (0, 2)] and run_of(1, caps, T) == [(0, 3), (1, 0), (1, 1)]
    assert run_of(10924, caps, T) == [(2, 0), (2, 1), (2, 2)] and run_of(10925, caps, T) == []
    assert ns[0] == caps[0] and ns[0] - 3 * T == 5 and 2 * T < ns[1] and ns[1] % T and ns[2] == caps[2] and all(n <= c for n, c in zip(ns, caps))
    return caps


def run_lags(shafa):
    """one, two and three lags; the middle block's are both at least PLANES_LAG_STRIP, so with its 2^28 capacity its chunks are
    m > 1 rounds long in the first pass (LAG_PLANES_SKIP) and in the pass in place (LAG_ELEMS), and its size is three of the
    longer chunks and a bit: the sums and the scan passes run"""
    strip = shafa.PLANES_LAG_STRIP
    rows = [(3,), (strip + 3, 2 * strip + 5), (1, 37, strip + 44)]
    geoms = [lag._geom(shafa, BIG_CAP, g) for g in rows[1]]
    assert all(g[3] > 1 for g in geoms)
    mid = max(3 * g[4] * L + L + 7 for g, L in zip(geoms, rows[1]))
    assert all(lag._geom(shafa, BIG_CAP, L)[4] * L * 3 < mid for L in rows[1])
    return rows, mid


def run_sizes(shafa):
    T = shafa.PLANES_TILE
    rows, mid = run_lags(shafa)
    ns = [3 * T + 5, mid, 20000]
    return rows, ns, assert_runs(T, ns)


def error_run_blocks(shafa, entry, k):
    """three blocks that differ in alignment, format, parameters and (pair) in the alignment of h_ref_off"""
    T = shafa.PLANES_TILE
    ns = [3 * T + 5, 5 * T + 77, 20000]
    fmts = [q.FMTS[k][j % len(q.FMTS[k])] for j in range(3)]
    out = []
    for j, (n, fmt, a) in enumerate(zip(ns, fmts, A_OFF[k])):
        b = dict(name=f"n={n}", fmt=fmt, a=a, x=q._values(n, fmt, T, 3 + j))
        if entry == "round":
            b["keep"] = (2, q.MANT[fmt] // 2, 0)[j]
        elif entry == "quant":
            step = (2.0 ** -10, fld._exact(0.37, k), 3.0)[j]
            b.update(step=step, bound=fld._exact(step * (0.5 + 2.0 ** -6), k))
        else:
            b.update(y=came_back(b["x"], fmt, j), abs=(1e-3, 0.0, 0.5)[j], rel=(0.0, 2.0 ** -6, 2.0 ** -4)[j])
        out.append(b)
    assert k != 2 or {b["fmt"] for b in out} == {"bfloat16", "float16"}
    assert len({b["a"] for b in out}) == min(3, 16 // k) and (k != 4 or 2 in {b["a"] for b in out})
    return out


@pytest.mark.parametrize("entry,k", ENTRIES)
def test_error_runs_of_tiles_per_workgroup(shafa, entry, k):
    T = shafa.PLANES_TILE
    blks = _once(("error runs", entry, k), lambda: error_run_blocks(shafa, entry, k))
    caps = assert_runs(T, [b["x"].size for b in blks])
    _launch(shafa, entry, k, blks, caps)


def _grid_run(shafa, k):
    rows, ns, caps = run_sizes(shafa)
    blocks = [(n, s, a) for n, s, a in zip(ns, rows, A_OFF[k])]
    return blocks, caps, _once(("grid runs", k), lambda: grd._Layout(k, blocks, 11000 + k))


@pytest.mark.parametrize("k", eal.ELEMS)
def test_grid_split_runs_of_tiles_per_workgroup(shafa, k):
    blocks, caps, L = _grid_run(shafa, k)
    st, bt = eal._batch(shafa, 3)
    try:
        d_el, d_pl = lag._to(L.el), lag._fill(L.pl.size)
        assert [(d_el.data_ptr() + o) % 16 for o in L.off] == [a * k % 16 for _, _, a in blocks]
        bt.split_planes_grid_dev(st, k, L.lags, d_el, L.off, caps, eal._dn(L.n), d_pl, L.poff)
        assert bt.finish(st, 3) == (0, [0] * 3), k
        eal._same_image(d_pl, L.pl, L.poff, k, blocks, f"grid split, E = {k}, planes; blocks are (n, lags, a)")
        eal._same_image(d_el, L.el, L.off, 1, blocks, f"grid split, E = {k}, the input; blocks are (n, lags, a)")
    finally:
        bt.close()


@pytest.mark.parametrize("k", eal.ELEMS)
def test_grid_merge_runs_of_tiles_per_workgroup(shafa, k):
    """block 0 (lag 3) and block 1 go through planes_lag_sums / _scan / _merge<E, LAG_PLANES_SKIP>, block 2 (first lag 1) through
    the difference merge; blocks 1 and 2 then through the passes in place <E, LAG_ELEMS>.  The sums scratch is 1024 k bytes a
    tile of the capacities: 268 MB at k = 8"""
    blocks, caps, L = _grid_run(shafa, k)
    st, bt = eal._batch(shafa, 3)
    try:
        d_pl, d_out = lag._to(L.pl), lag._fill(L.el.size)
        assert [(d_out.data_ptr() + o) % 16 for o in L.off] == [a * k % 16 for _, _, a in blocks]
        bt.merge_planes_grid_dev(st, k, L.lags, d_pl, L.poff, caps, eal._dn(L.n), d_out, L.off)
        assert bt.finish(st, 3) == (0, [0] * 3), k
        eal._same_image(d_out, L.el, L.off, 1, blocks, f"grid merge, E = {k}, elements; blocks are (n, lags, a)")
        eal._same_image(d_pl, L.pl, L.poff, k, blocks, f"grid merge, E = {k}, the planes; blocks are (n, lags, a)")
    finally:
        bt.close()


class _QuantLayout(fld._Layout):
    """test_gpu_fields._Layout over elements the caller brings (xs)"""

    def __init__(self, shafa, k, blocks, xs):
        self.k, self.n, self.lags = k, [b[0] for b in blocks], [tuple(b[1]) for b in blocks]
        self.step, self.bound = [b[3] for b in blocks], [b[4] for b in blocks]
        self.off, self.poff, self.x = [], [], []
        pos, ppos = 0, 16
        for n, _, a, _, _ in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + a * k
            self.off.append(pos)
            pos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += lag._al16(n) + 32
        self.el = np.full(pos + 80, lag.FILL, np.uint8)
        self.pl = np.full(ppos + 16, lag.FILL, np.uint8)
        self.out = self.el.copy()
        self.rec, self.good = [], []
        for b, ((n, lags, _, step, bound), x) in enumerate(zip(blocks, xs)):
            assert x.dtype == fld.FLOAT[k] and x.size == n
            code, xr, good = fld._model(x, step, bound)
            sl = slice(self.off[b], self.off[b] + n * k)
            self.el[sl] = x.view(np.uint8)
            self.out[sl] = fld._restored(x, xr, good).view(np.uint8)
            planes = grd._z_planes(code.tobytes(), k, lags)
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = planes[j]
            self.x.append(x)
            self.rec.append(fld._records(x, good))
            self.good.append(good)


def quant_run_blocks(shafa, k):
    """(blocks (n, lags, a, step, bound), xs): outliers some, none, some — the middle block is test_gpu_fields._values' ramp
    without what it plants"""
    T = shafa.PLANES_TILE
    rows, ns, _ = run_sizes(shafa)
    steps = [2.0 ** -10, fld._exact(0.37, k), 3.0]
    blocks = [(n, s, a, st, fld._exact(st * (0.5 + 2.0 ** -6), k)) for n, s, a, st in zip(ns, rows, A_OFF[k], steps)]
    xs = [fld._values(n, k, b[3], T, 7 + j) for j, (n, b) in enumerate(zip(ns, blocks))]
    i = np.arange(ns[1], dtype=np.float64)
    xs[1] = ((0.37 * (i % 4096) + 40 * np.sin(i / 11) + 8) * steps[1]).astype(fld.FLOAT[k])
    return blocks, xs


def _quant_run(shafa, k):
    def make():
        blocks, xs = quant_run_blocks(shafa, k)
        return blocks, _QuantLayout(shafa, k, blocks, xs)
    blocks, L = _once(("quant runs", k), make)
    found = [len(r) for r in L.rec]
    assert found[0] > 3 and found[1] == 0 and found[2] > 3
    return blocks, run_sizes(shafa)[2], L, found


def _freq_of(L):
    """np.bincount over every plane of the layout: [nb * k * 256]"""
    out = np.zeros(len(L.poff) * 256, np.uint64)
    for r, o in enumerate(L.poff):
        out[r * 256:(r + 1) * 256] = np.bincount(L.pl[o:o + L.n[r // L.k]], minlength=256)
    return out


def _field_split(shafa, kind, L, caps, show, classes=None):
    """one launch of the quantising ("quant") or the rounding ("round") split over the layout's blocks: the planes, the counts
    with their guards and the sorted records, every buffer whole; the input comes back unchanged"""
    k, nb = L.k, len(L.n)
    found = [len(r) for r in L.rec]
    ooff, room = eal._record_places(L.n)
    st, bt = eal._batch(shafa, nb)
    try:
        d_el, d_pl, d_outl, d_cnt = lag._to(L.el), lag._fill(L.pl.size), fld._fill64(2 * room), fld._fill64(nb + 2)
        addr = [d_el.data_ptr() + o for o in L.off]
        assert [p % 16 for p in addr] == [b[2] * k % 16 for b in show] and d_pl.data_ptr() % 16 == 0
        if classes is not None:
            classes(addr)
        if kind == "quant":
            bt.split_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, caps, eal._dn(L.n), d_pl, L.poff, d_outl, ooff,
                                           L.n, d_cnt[1:nb + 1])
        else:
            bt.split_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, caps, eal._dn(L.n), d_pl, L.poff, d_outl, ooff,
                                           L.n, d_cnt[1:nb + 1])
        assert bt.finish(st, nb) == (0, [0] * nb), (kind, k)
        eal._same_image(d_pl, L.pl, L.poff, k, show, f"{kind} split, E = {k}, planes; blocks are (n, lags, a)")
        eal._same_image(d_el, L.el, L.off, 1, show, f"{kind} split, E = {k}, the input; blocks are (n, lags, a)")
        cnt = d_cnt.tolist()
        bad = [(show[b], cnt[b + 1], found[b]) for b in range(nb) if cnt[b + 1] != found[b]]
        assert not bad, f"{kind} split, E = {k}: (block (n, lags, a), outliers counted, the model's) {bad[:4]}"
        assert cnt[0] == cnt[-1] == fld.FILL64 - (1 << 64)
        rec = fld._rec_img(d_outl)
        want = np.full_like(rec, fld.FILL64)
        for b in range(nb):
            rec[ooff[b]:ooff[b] + found[b]] = fld._sorted(rec[ooff[b]:ooff[b] + found[b]])
            want[ooff[b]:ooff[b] + found[b]] = L.rec[b]
            assert rec[ooff[b]:ooff[b] + found[b]].tobytes() == L.rec[b].tobytes(), f"{kind} split, E = {k}: records of block {show[b]}"
        assert rec.tobytes() == want.tobytes(), (kind, k)
    finally:
        bt.close()


def _field_merge(shafa, kind, L, caps, show, classes=None):
    """one launch of the family's merge from numpy's planes and the model's records: the grid merge's chain, the restore pass in
    place, then the patch; the elements whole, the planes and the records back unchanged"""
    import torch
    k, nb = L.k, len(L.n)
    found = [len(r) for r in L.rec]
    ooff, room = eal._record_places(L.n)
    recs = np.full((room, 2), fld.FILL64, np.uint64)
    for b in range(nb):
        recs[ooff[b]:ooff[b] + found[b]] = L.rec[b]
    st, bt = eal._batch(shafa, nb)
    try:
        d_pl, d_out = lag._to(L.pl), lag._fill(L.el.size)
        d_rec = lag._to(recs.view(np.int64).reshape(-1))
        addr = [d_out.data_ptr() + o for o in L.off]
        assert [p % 16 for p in addr] == [b[2] * k % 16 for b in show] and d_pl.data_ptr() % 16 == 0
        if classes is not None:
            classes(addr)
        if kind == "quant":
            bt.merge_planes_grid_quant_dev(st, k, L.lags, L.step, d_pl, L.poff, caps, eal._dn(L.n), d_rec, ooff, found, d_out, L.off)
        else:
            bt.merge_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_pl, L.poff, caps, eal._dn(L.n), d_rec, ooff, found, d_out,
                                           L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), (kind, k)
        eal._same_image(d_out, L.out, L.off, 1, show, f"{kind} merge, E = {k}, elements; blocks are (n, lags, a)")
        eal._same_image(d_pl, L.pl, L.poff, k, show, f"{kind} merge, E = {k}, the planes; blocks are (n, lags, a)")
        assert lag._img(d_rec.view(torch.uint8)) == recs.tobytes(), (kind, k)
    finally:
        bt.close()


def _field_hist(shafa, kind, L, caps, show, classes=None):
    """one launch of the family's histogram entry: the counts against np.bincount over numpy's planes and the outlier counts
    against the model's, both between guard words; the input comes back unchanged"""
    k, nb = L.k, len(L.n)
    found = [len(r) for r in L.rec]
    freq = _once(("freq", id(L)), lambda: _freq_of(L))
    st, bt = eal._batch(shafa, nb)
    try:
        d_el, d_freq, d_cnt = lag._to(L.el), fld._fill64(nb * k * 256 + 2), fld._fill64(nb + 2)
        addr = [d_el.data_ptr() + o for o in L.off]
        assert [p % 16 for p in addr] == [b[2] * k % 16 for b in show]
        if classes is not None:
            classes(addr)
        if kind == "quant":
            bt.hist_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, caps, eal._dn(L.n), d_freq[1:-1], d_cnt[1:nb + 1])
        else:
            bt.hist_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, caps, eal._dn(L.n), d_freq[1:-1], d_cnt[1:nb + 1])
        assert bt.finish(st, nb) == (0, [0] * nb), (kind, k)
        hf = d_freq.cpu().numpy().view(np.uint64)
        bad = [show[b] for b in range(nb) if hf[1 + b * k * 256:1 + (b + 1) * k * 256].tobytes() != freq[b * k * 256:(b + 1) * k * 256].tobytes()]
        assert not bad, f"{kind} histograms, E = {k}: blocks (n, lags, a) {bad[:6]}"
        assert hf[0] == fld.FILL64 and hf[-1] == fld.FILL64 and hf[1:-1].tobytes() == freq.tobytes(), (kind, k)
        assert d_cnt.tolist() == [fld.FILL64 - (1 << 64)] + found + [fld.FILL64 - (1 << 64)], (kind, k)
        eal._same_image(d_el, L.el, L.off, 1, show, f"{kind} histograms, E = {k}, the input; blocks are (n, lags, a)")
    finally:
        bt.close()


@pytest.mark.parametrize("k", eal.FIELD_ELEMS)
def test_quant_split_runs_of_tiles_per_workgroup(shafa, k):
    blocks, caps, L, _ = _quant_run(shafa, k)
    _field_split(shafa, "quant", L, caps, [b[:3] for b in blocks])


@pytest.mark.parametrize("k", eal.FIELD_ELEMS)
def test_quant_merge_runs_of_tiles_per_workgroup(shafa, k):
    """numpy's planes and the model's records: the grid merge's chain, planes_field_restore, then the patch"""
    blocks, caps, L, _ = _quant_run(shafa, k)
    _field_merge(shafa, "quant", L, caps, [b[:3] for b in blocks])


def round_run_blocks(shafa, k):
    """(n, lags, a, format, keep): both 16-bit formats in one launch; keep = mant in the middle leaves no outlier, keep 0 and 2
    leave the denormals and the NaNs whose payload is dropped"""
    rows, ns, _ = run_sizes(shafa)
    fmts = [q.FMTS[k][j % len(q.FMTS[k])] for j in (0, 1, 0)]
    keeps = [2, rnd.MANT[fmts[1]], 0]
    return [(n, s, a, f, kp) for n, s, a, f, kp in zip(ns, rows, A_OFF[k], fmts, keeps)]


def _round_run(shafa, k):
    blocks = round_run_blocks(shafa, k)
    L = _once(("round runs", k), lambda: rnd._Layout(shafa, blocks, 11100 + k))
    found = [len(r) for r in L.rec]
    assert found[0] > 3 and found[1] == 0 and found[2] > 3 and (k != 2 or set(L.mant) == {7, 10})
    return [b[:3] for b in blocks], run_sizes(shafa)[2], L


@pytest.mark.parametrize("k", (2, 4, 8))
def test_round_split_runs_of_tiles_per_workgroup(shafa, k):
    show, caps, L = _round_run(shafa, k)
    _field_split(shafa, "round", L, caps, show)


@pytest.mark.parametrize("k", (2, 4, 8))
def test_round_merge_runs_of_tiles_per_workgroup(shafa, k):
    """the grid merge's chain, planes_round_restore, then the patch"""
    show, caps, L = _round_run(shafa, k)
    _field_merge(shafa, "round", L, caps, show)


# ---------------------------------------------------------------- B. long blocks in planes_error_blocks
def fold_threads(n, T):
    """(per, the threads that hold a partial, the partials of the last of them)"""
    nt = -(-n // T)
    per = -(-nt // THREADS)
    held = -(-nt // per)
    return per, held, nt - (held - 1) * per


def _span8(n, fmt, seed):
    """test_gpu_quality._values' ramp over the binades 2^-8 .. 2^8 with both signs: every |x| is below 512"""
    i = np.arange(n, dtype=np.float64)
    v = (1.0 + 0.37 * np.sin(i / 11 + seed)) * 2.0 ** (8 * np.sin(i / 301 + 0.1 * seed)) * np.where((i // 7) % 3 == 1, -1.0, 1.0)
    return q._to_bits(v, fmt).copy()


def _borders(x, fmt, T, keep_last=False):
    """NaN and +-Inf on both sides of tile borders inside a long block: the borders of a thread's run at per = 1, 2 and 3"""
    SIGN, INF, MIN = q._consts(fmt)
    nonfin = [INF, INF | (MIN >> 1), SIGN | INF, SIGN | INF | 1]
    for j, at in enumerate((0, T - 1, T, T + 1, 2 * T - 1, 3 * T, 128 * T - 1, 128 * T, 255 * T, 256 * T - 1, 256 * T, 512 * T - 1, 512 * T)):
        if at < x.size - (2 if keep_last else 0):
            x[at] = x.dtype.type(nonfin[j % 4])
    return x


def _entry_params(entry, fmt):
    """the planted blocks' parameters, test_gpu_quality's: at keep 1 the element 1280 is an exact tie and comes back as 1024, at
    step 0.5 the element 1.25 comes back as 1.0; the pair's y is the rounding rule's four bits
    below half the mantissa (at float64 e e then rounds), 1536 at a plant"""
    if entry == "round":
        return dict(keep=1), 1280.0, 256.0
    if entry == "quant":
        return dict(step=0.5, bound=0.25), 1.25, 0.25
    return dict(abs=1e-3, rel=2.0 ** -9), 1280.0, 256.0


def _back(entry, x, fmt, p, plants):
    if entry == "round":
        return q._round(x, q.MANT[fmt], p["keep"])[0]
    if entry == "quant":
        return q._quant(x, p["step"], p["bound"])[0]
    y = q._round(x, q.MANT[fmt], max(q.MANT[fmt] // 2 - 4, 0))[0].copy()
    y[plants] = q._to_bits(np.array([1536.0]), fmt)[0]
    return y


def planted_block(entry, fmt, T, n, seed, a, last_only):
    """a block of n elements of _span8 data whose largest e stands at `plants` alone: three times at one value (tile 2, tile 3,
    tile 400), or at the very last element only.  The first kind has its minimum in the first and its maximum in the last tile."""
    p, big, e_big = _entry_params(entry, fmt)
    bits = lambda v: q._to_bits(np.array([v]), fmt)[0]
    plants = [n - 1] if last_only else [2 * T + 100, 3 * T + 7, 400 * T + 4096 + 33]
    x = _borders(_span8(n, fmt, seed), fmt, T, keep_last=True)
    x[plants] = bits(big)
    ends = [] if last_only else [5, n - 3]
    if ends:
        x[ends] = [bits(-16384.0), bits(16384.0)]
    # no other element reaches the planted error
    dx, dy = q._dbl(x, fmt), q._dbl(_back(entry, x, fmt, p, plants), fmt)
    with np.errstate(all="ignore"):
        reach = np.isfinite(dx) & np.isfinite(dy) & (np.abs(dx - dy) >= e_big)
    reach[plants] = False
    x[reach] = bits(1.0)
    b = dict(name="largest last" if last_only else "largest thrice, min first, max last", fmt=fmt, a=a, x=x, plants=plants, e_big=e_big,
             ends=ends, **p)
    if entry == "pair":
        b["y"] = _back(entry, x, fmt, p, plants)
    return b


def assert_plants(b, want):
    assert want[9] == b["plants"][0] and want[8] == q._b(b["e_big"]), (b["name"], want)
    assert want[1] > 0.99 * b["x"].size and want[2] >= 6
    if b["ends"]:
        assert (want[10], want[11]) == (q._b(-16384.0), q._b(16384.0)), (b["name"], want)


def long_blocks(shafa, entry, k):
    T = shafa.PLANES_TILE
    fmts = q.FMTS[k]
    n3 = 513 * T + 5
    out = []
    if k == 2:                                                             # per = 1 and per = 2, a format each
        for j, n in enumerate((256 * T, 256 * T + 1)):
            fmt = fmts[j]
            out.append(dict(name=f"n={n}", fmt=fmt, a=1 + j, x=_borders(q._values(n, fmt, T, 1 + j), fmt, T), keep=(3, 5)[j]))
    out.append(planted_block(entry, fmts[0], T, n3, 4, 3 % (16 // k), False))
    out.append(planted_block(entry, fmts[-1], T, n3, 5, 0, True))
    fmt = fmts[-1]
    p = _entry_params(entry, fmt)[0]
    x = q._values(17, fmt, T, 6)
    out.append(dict(name="n=17", fmt=fmt, a=1, x=x, **p))
    if entry == "pair":
        out[-1]["y"] = q._came_back(x, fmt, 1)
    return out


LONG = (("round", 2), ("quant", 4), ("pair", 8))


def assert_long(T, blks, k):
    pers = [fold_threads(b["x"].size, T) for b in blks]
    if k == 2:
        assert pers[:2] == [(1, 256, 1), (2, 129, 1)] and {b["fmt"] for b in blks} == {"bfloat16", "float16"}
    assert pers[-3:] == [(3, 172, 1), (3, 172, 1), (1, 1, 1)] and blks[-3]["x"].size == 513 * T + 5
    pl = blks[-3]["plants"]
    assert [p // T for p in pl] == [2, 3, 400] and [p // T // 3 for p in pl] == [0, 1, 133]          # the threads that fold them
    assert blks[-2]["plants"] == [513 * T + 4]
    assert blks[-3]["ends"][0] < T and blks[-3]["ends"][1] >= 513 * T


@pytest.mark.parametrize("entry,k", LONG)
def test_long_blocks_fold_per_1_2_3(shafa, entry, k):
    T = shafa.PLANES_TILE
    blks = _once(("long", entry, k), lambda: long_blocks(shafa, entry, k))
    assert_long(T, blks, k)
    for b in blks[-3:-1]:
        assert_plants(b, _want(entry, b, T)[1])
    _launch(shafa, entry, k, blks)


# ---------------------------------------------------------------- C. test_gpu_quality's table, all twelve words for equality
def quality_blocks(shafa, entry, k):
    T = shafa.PLANES_TILE
    if entry == "round":
        return [dict(name=b[0], fmt=b[1], a=b[2], x=b[3], keep=b[4]["keep"](q.MANT[b[1]])) for b in q._blocks(k, T, q._round_params())]
    if entry == "quant":
        return [dict(name=b[0], fmt=b[1], a=b[2], x=b[3], step=b[4]["step"], bound=b[4]["bound"])
                for b in q._blocks(k, T, q._quant_params(shafa, k))]
    out = []
    for j, b in enumerate(q._blocks(k, T, [dict(big=1280.0, small=q._small_round)] * 2)):
        bd = q.PAIR_BOUNDS[j % 5]
        out.append(dict(name=b[0], fmt=b[1], a=b[2], x=b[3], y=q._came_back(b[3], b[1], j, b[4].get("first")), abs=bd[0], rel=bd[1]))
    return out


@pytest.mark.parametrize("entry,k", ENTRIES)
def test_the_quality_table_bit_for_bit(shafa, entry, k):
    blks = _once(("quality", entry, k), lambda: quality_blocks(shafa, entry, k))
    assert any(b["x"].size == 2 * shafa.PLANES_TILE + 3 for b in blks) and any(b["x"].size == 0 for b in blks)
    _launch(shafa, entry, k, blks)


def fused_bound(abs_b, rel_b, x):
    """abs + rel |x| with ONE rounding, as a contracted multiply-add would give it"""
    return float(Fraction(abs_b) + Fraction(rel_b) * abs(Fraction(x)))


REL_ODD, ABS_ODD = 10.1, 2.3                                               # rel is no power of two: rel |x| rounds


def over_plants(counted=6, not_counted=2):
    """elements x = 1 + j 2^-20 below 1.5 at which abs + rel |x| differs by its last bit between two roundings and one, and
    y = x - the larger of the two, exact: e IS the larger bound, so it is past the smaller one only -> [(x, y, over as the header
    counts it, over if the bound were contracted)], `counted` of the first kind and `not_counted` of the second"""
    out = []
    left = {True: counted, False: not_counted}
    j = 0
    while left[True] or left[False]:
        j += 1
        x = 1.0 + j * 2.0 ** -20
        assert x < 1.5
        two, one = ABS_ODD + REL_ODD * x, fused_bound(ABS_ODD, REL_ODD, x)
        if two == one:
            continue
        hi = max(two, one)
        y = x - hi
        assert Fraction(x) - Fraction(hi) == Fraction(y) and abs(x - y) == hi
        if not left[hi > two]:
            continue
        left[hi > two] -= 1
        out.append((x, y, hi > two, hi > one))
    return out


def overflow_blocks(shafa):
    """float64 through error_dev: |x| around 1e200 (x x overflows: word 7 is +Inf), a pair 1.5e308 / -1.5e308 that is finite on
    both sides with e = +Inf, and the elements of over_plants under a bound that rounds twice"""
    T = shafa.PLANES_TILE
    fmt = "float64"
    n = 2 * T + 3
    i = np.arange(n, dtype=np.float64)
    x = 1e200 * (1.0 + 0.37 * np.sin(i / 11)) * np.where((i // 7) % 3 == 1, -1.0, 1.0)
    y = x.copy()
    y.view(np.uint64)[::3] ^= np.uint64(1)
    huge = dict(name="1e200", fmt=fmt, a=1, x=x.view(np.uint64), y=y.view(np.uint64), abs=1e180, rel=0.0)
    x = q._dbl(_span8(T + 17, fmt, 2), fmt)
    y = x.copy()
    x[4321], y[4321] = 1.5e308, -1.5e308
    inf_e = dict(name="e = Inf", fmt=fmt, a=0, x=x.view(np.uint64), y=y.view(np.uint64), abs=0.5, rel=0.0)
    x = 1.0 + (np.arange(100) % 50) / 64.0
    y = x.copy()
    plants = over_plants()
    for j, (px, py, _, _) in enumerate(plants):
        x[7 + 11 * j], y[7 + 11 * j] = px, py
    odd = dict(name="a bound that rounds twice", fmt=fmt, a=1, x=x.view(np.uint64), y=y.view(np.uint64), abs=ABS_ODD, rel=REL_ODD)
    return [huge, inf_e, odd], plants


def test_overflow_and_the_bound_of_word_5(shafa):
    T = shafa.PLANES_TILE
    blks, plants = _once("overflow", lambda: overflow_blocks(shafa))
    w = [_want("pair", b, T)[1] for b in blks]
    assert w[0][7] == INF_BITS and w[0][1] == 2 * T + 3
    assert w[1][6] == INF_BITS and w[1][8] == INF_BITS and w[1][9] == 4321 and w[1][2] == 0 and w[1][5] == 1
    assert w[2][5] == sum(p[2] for p in plants) != sum(p[3] for p in plants)
    _launch(shafa, "pair", 8, blks)


# ---------------------------------------------------------------- D. the error entries at every alignment of the x side
def error_align_blocks(shafa, entry, k):
    """(n, a): the x side at every multiple of k below 16, crossed with the counts 1 .. 17 and T - 1, T + 1"""
    T = shafa.PLANES_TILE
    fmts = q.FMTS[k]
    out = []
    for j, (a, n) in enumerate((a, n) for a in eal.aligns(k) for n in tuple(range(1, 18)) + (T - 1, T + 1)):
        fmt = fmts[(j + j // 19) % len(fmts)]
        b = dict(name=f"n={n}, a={a}", fmt=fmt, a=a, x=q._values(n, fmt, T, j % 11))
        if entry == "round":
            m = q.MANT[fmt]
            b["keep"] = (0, 1, m // 2, m - 1, m)[j % 5]
        elif entry == "quant":
            step = (2.0 ** -10, fld._exact(1e-3, k), fld._exact(0.37, k), 3.0)[j % 4]
            b.update(step=step, bound=fld._exact(step * (0.5 + 2.0 ** -6), k))
        else:
            bd = q.PAIR_BOUNDS[j % 5]
            b.update(y=came_back(b["x"], fmt, j), abs=bd[0], rel=bd[1])
        out.append(b)
    return out


def assert_error_aligns(blks, k, T, addr=None):
    """every (alignment, count) pair, and with it every instantiation Q of err_tile at every byte shift r"""
    addr = [b["a"] * k for b in blks] if addr is None else addr
    counts = set(range(1, 18)) | {T - 1, T + 1}
    assert {(p % 16, b["x"].size) for p, b in zip(addr, blks)} == {(A, n) for A in range(0, 16, k) for n in counts}
    eal._assert_own(addr, k)
    assert k != 2 or {(p % 16, b["fmt"]) for p, b in zip(addr, blks)} == {(A, f) for A in range(0, 16, 2) for f in q.FMTS[2]}


@pytest.mark.parametrize("entry,k", ENTRIES)
def test_error_entries_at_every_alignment(shafa, entry, k):
    """error_dev's y side stays at multiples of 16, as the API demands"""
    T = shafa.PLANES_TILE
    blks = _once(("error aligns", entry, k), lambda: error_align_blocks(shafa, entry, k))
    _launch(shafa, entry, k, blks, classes=lambda addr: assert_error_aligns(blks, k, T, addr))


# ---------------------------------------------------------------- D. the rounding kernels and the two new histograms
def _behind(D, rho):
    """the two smallest counts past D that are rho mod 16"""
    n = D + 1 + (rho - D - 1) % 16
    return n, n + 16


def round_align_blocks(shafa, k):
    """(n, lags, a, format, keep).  First one lag 1 .. 16 at every alignment with two counts: every (own, tap) pair, every byte
    count of the zeroed head at each, and at each alignment every last-unit count 1 .. 16.  Then the quantiser's table of
    test_gpu_every_alignment_lag.py: its lag sets (taps on sub_words' and on add_words' side) at the counts 0 .. 17, 33, T - 1,
    T, T + 1, 2 T + 3: the restore pass's cut words at every (start, end) mod 16.  Formats and kept bits go round."""
    T = shafa.PLANES_TILE
    small = [(n, (D,), a) for a in eal.aligns(k) for D in range(1, 17) for n in _behind(D, (7 * D + a) % 16)]
    counts = tuple(range(18)) + (33, T - 1, T, T + 1, 2 * T + 3)
    big = [(n, s, a) for a in eal.aligns(k) for s in eal.QUANT_SETS(T) for n in counts]
    kinds = [(f, kp) for f in q.FMTS[k] for kp in (0, 1, rnd.MANT[f] // 2, rnd.MANT[f] - 1, rnd.MANT[f])]
    return [r + kinds[(b + b // len(kinds)) % len(kinds)] for b, r in enumerate(small + big)], len(small)


def assert_round_classes(addr, blocks, n_small, k, T, cut=False):
    show = [b[:3] for b in blocks]
    eal._assert_grid_classes(addr, show, k)
    small = [(p, s[0]) for p, (n, s, _) in zip(addr[:n_small], show[:n_small])]
    assert all(D < n for (n, (D,), _) in show[:n_small])
    eal._assert_heads(small, k)
    for A in range(0, 16, k):                                              # the last unit's count at every alignment
        assert {n % 16 for p, (n, _, _) in zip(addr[:n_small], show) if p % 16 == A} == set(range(16)), (k, A)
    assert k != 2 or {(p % 16, b[3]) for p, b in zip(addr, blocks)} == {(A, f) for A in range(0, 16, 2) for f in q.FMTS[2]}
    if cut:
        eal._assert_cut_words(addr, show, k, T)


def _round_align(shafa, k):
    blocks, n_small = round_align_blocks(shafa, k)
    return blocks, n_small, _once(("round aligns", k), lambda: rnd._Layout(shafa, blocks, 11200 + k))


@pytest.mark.parametrize("k", (2, 4, 8))
def test_round_split_at_every_alignment(shafa, k):
    blocks, n_small, L = _round_align(shafa, k)
    T = shafa.PLANES_TILE
    _field_split(shafa, "round", L, eal._caps(L.n), [b[:3] for b in blocks], lambda addr: assert_round_classes(addr, blocks, n_small, k, T))


@pytest.mark.parametrize("k", (2, 4, 8))
def test_round_merge_at_every_alignment(shafa, k):
    blocks, n_small, L = _round_align(shafa, k)
    T = shafa.PLANES_TILE
    _field_merge(shafa, "round", L, eal._caps(L.n), [b[:3] for b in blocks],
                 lambda addr: assert_round_classes(addr, blocks, n_small, k, T, cut=True))


@pytest.mark.parametrize("k", (2, 4, 8))
def test_round_histograms_at_every_alignment(shafa, k):
    blocks, n_small, L = _round_align(shafa, k)
    T = shafa.PLANES_TILE
    _field_hist(shafa, "round", L, eal._caps(L.n), [b[:3] for b in blocks], lambda addr: assert_round_classes(addr, blocks, n_small, k, T))


@pytest.mark.parametrize("k", eal.FIELD_ELEMS)
def test_quant_histograms_at_every_alignment(shafa, k):
    """the quantiser's table of test_gpu_every_alignment_lag.py, and its layout"""
    blocks, L = eal._quant(shafa, k)
    show = [b[:3] for b in blocks]
    _field_hist(shafa, "quant", L, eal._caps(L.n), show, lambda addr: eal._assert_grid_classes(addr, show, k))
