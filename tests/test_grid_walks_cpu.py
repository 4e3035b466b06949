"""The block tables and the fold model of tests/test_gpu_grid_walks.py hold what that file claims (no GPU needed).

The tables: the run arithmetic (three tiles a workgroup, workgroup 1 ends block 0 and starts block 1), the long blocks' per = 1, 2
and 3 and the threads that fold the plants, the alignment tables' classes over the addresses a * k.  Thinning a table fails here.

The model: exact_sum is checked against a scalar restatement of the header's order, and the comparison for equality is shown not
to be vacuous for the inputs the GPU tests use: the model differs in bits from a sequential sum, from the tree taken from 32 down
to 1 and from a fold that takes a thread's first partial only; contracting the product into the sum changes nothing at two and
four bytes (the products are exact in double) and changes lane sums at float64 (exact rational arithmetic on one tile); and the
planted elements of word 5 fall on the other side of a bound that is rounded once instead of twice."""
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_every_alignment_lag as eal
import test_gpu_grid_walks as gw
import test_gpu_planes_lag as lag
import test_gpu_quality as q

FMTS = ("bfloat16", "float16", "float32", "float64")


# ---------------------------------------------------------------- A. runs of tiles per workgroup
def test_three_tiles_a_workgroup_and_a_run_across_two_blocks(shafa):
    T, strip = shafa.PLANES_TILE, shafa.PLANES_LAG_STRIP
    rows, ns, caps = gw.run_sizes(shafa)
    assert caps == [3 * T + 5, 1 << 28, 20000] and [-(-c // T) for c in caps] == [4, 32768, 3]
    assert gw.run_of(1, caps, T) == [(0, 3), (1, 0), (1, 1)] and gw.run_of(2, caps, T) == [(1, 2), (1, 3), (1, 4)]
    assert gw.run_of(10923, caps, T) == [(1, 32765), (1, 32766), (1, 32767)]
    assert [len(s) for s in rows] == [1, 2, 3] and min(rows[1]) >= strip and rows[2][0] == 1 and rows[0][0] != 1
    assert any(g >= strip for g in rows[2][1:]) and any(g < strip for g in rows[2][1:])
    # the middle block: chunks of more than one round in both of its passes, three of them and a bit
    for L in rows[1]:
        g = lag._geom(shafa, caps[1], L)
        assert g[3] > 1 and 3 * g[4] * L < ns[1] < 5 * g[4] * L
    assert ns[1] > 2 * T and ns[1] % T
    for bad in ([ns[0] - 5, ns[1], ns[2]], [ns[0], T, ns[2]], [ns[0], 2 * T, ns[2]]):
        with pytest.raises(AssertionError):
            gw.assert_runs(T, bad)
    for k in eal.ELEMS:
        assert len(set(gw.A_OFF[k])) == min(3, 16 // k) and all(a * k < 16 for a in gw.A_OFF[k])
    assert 2 in gw.A_OFF[4]                                                # Q = 2 at four bytes


def test_the_blocks_of_a_run_differ_in_what_a_block_owns(shafa):
    T = shafa.PLANES_TILE
    for entry, k in gw.ENTRIES:
        blks = gw.error_run_blocks(shafa, entry, k)
        gw.assert_runs(T, [b["x"].size for b in blks])
        key = {"round": lambda b: (b["fmt"], b["keep"]), "quant": lambda b: (b["step"], b["bound"]), "pair": lambda b: (b["abs"], b["rel"])}
        assert len({key[entry](b) for b in blks}) == 3, (entry, k)
        assert len({b["a"] * k % 16 for b in blks}) == min(3, 16 // k)
        assert k != 2 or {b["fmt"] for b in blks} == {"bfloat16", "float16"}
    for k in (4, 8):
        blocks, xs = gw.quant_run_blocks(shafa, k)
        assert len({b[3] for b in blocks}) == 3 and [b[2] for b in blocks] == list(gw.A_OFF[k])
        L = gw._QuantLayout(shafa, k, blocks, xs)
        found = [len(r) for r in L.rec]
        assert found[0] > 3 and found[1] == 0 and found[2] > 3
    for k in (2, 4, 8):
        blocks = gw.round_run_blocks(shafa, k)
        assert len({(b[3], b[4]) for b in blocks}) == 3 and (k != 2 or {b[3] for b in blocks} == {"bfloat16", "float16"})


# ---------------------------------------------------------------- B. long blocks
def test_long_blocks_per_1_2_3_and_the_threads_of_the_plants(shafa):
    T = shafa.PLANES_TILE
    assert gw.fold_threads(256 * T, T) == (1, 256, 1) and gw.fold_threads(256 * T + 1, T) == (2, 129, 1)
    assert gw.fold_threads(513 * T + 5, T) == (3, 172, 1) and gw.fold_threads(2 * T + 3, T) == (1, 3, 1)
    assert 256 * T + 1 > 2097152                                           # per >= 2 needs more than 2 097 152 elements
    for entry, k in gw.LONG:
        blks = gw.long_blocks(shafa, entry, k)
        gw.assert_long(T, blks, k)
        with pytest.raises(AssertionError):
            gw.assert_long(T, blks[:-3] + blks[-2:], k)
    entry, k = "quant", 4
    blks = gw.long_blocks(shafa, entry, k)
    for b in blks[-3:-1]:
        gw.assert_plants(b, gw._want(entry, b, T)[1])


# ---------------------------------------------------------------- C. the model
def _scalar_tree(v):
    d = 1
    while d < 64:
        v = [v[l] + v[l + d] if l + d < 64 else v[l] for l in range(64)]
        d *= 2
    return v[0]


def _scalar_reduce(lanes):
    w = [_scalar_tree(lanes[64 * j:64 * j + 64]) for j in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _scalar_sum(term, fin, T):
    """the header's order with Python floats, one operation at a time"""
    term, fin = term.tolist(), fin.tolist()
    n = len(term)
    parts = []
    for lo in range(0, n, T):
        lanes = []
        for lane in range(256):
            a = 0.0
            for u in range(T // 4096):
                for i in range(16):
                    j = lo + u * 4096 + lane * 16 + i
                    if j < n and fin[j]:
                        a = a + term[j]
            lanes.append(a)
        parts.append(_scalar_reduce(lanes))
    per = -(-len(parts) // 256)
    lanes = []
    for t in range(256):
        a = 0.0
        for p in parts[t * per:(t + 1) * per]:
            a = a + p
        lanes.append(a)
    return _scalar_reduce(lanes)


def _terms(xb, fmt):
    x = q._dbl(xb, fmt)
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        return x * x, fin


@pytest.mark.parametrize("fmt", FMTS)
def test_the_model_is_the_headers_order(shafa, fmt):
    T = shafa.PLANES_TILE
    term, fin = _terms(q._values(2 * T + 3, fmt, T, 8), fmt)
    assert gw.exact_sum(term, fin, T) == _scalar_sum(term, fin, T)
    # 600 partials: per = 3, the last thread that holds any holds them all
    part = np.abs(np.sin(np.arange(600.0))) * 1e3
    lanes = [float((part[3 * t] + part[3 * t + 1]) + part[3 * t + 2]) for t in range(200)] + [0.0] * 56
    assert gw.block_fold(part) == _scalar_reduce(lanes)
    assert gw.exact_sum(np.zeros(0), np.zeros(0, bool), T) == 0.0


def _tree_down(a):
    """the distances taken from 32 down to 1"""
    a = a.copy()
    d = 32
    while d >= 1:
        a[..., :64 - d] = a[..., :64 - d] + a[..., d:]
        d >>= 1
    return a[..., 0]


def _other_orders(term, fin, T):
    """(sequential, the tree from 32 down to 1 in both kernels, a thread's first partial only)"""
    with np.errstate(all="ignore"):
        seq = float(np.cumsum(term[fin])[-1])
        lanes = gw.lane_sums(term, fin, T)
        part = gw._waves(_tree_down(lanes.reshape(-1, 4, 64)))
        per = -(-part.size // 256)
        p = np.zeros(per * 256)
        p[:part.size] = part
        acc = np.zeros(256)
        for j in range(per):
            acc = acc + p.reshape(256, per)[:, j]
        down = float(gw._waves(_tree_down(acc.reshape(4, 64))))
        part = gw.tile_partials(term, fin, T)
        p = np.zeros(per * 256)
        p[:part.size] = part
        first = float(gw._waves(gw._tree(p.reshape(256, per)[:, 0].copy().reshape(4, 64))))
    return seq, down, first


def _used_inputs(shafa):
    """(what, format, x): the blocks of two tiles and more, as the GPU tests build them"""
    T = shafa.PLANES_TILE
    out = []
    for k in (2, 4, 8):
        for b in gw.quality_blocks(shafa, "round", k) + gw.error_run_blocks(shafa, "round", k):
            if b["x"].size >= 2 * T and b["name"].startswith("n="):
                out.append((b["name"], b["fmt"], b["x"]))
    for entry, k in gw.LONG:
        for b in gw.long_blocks(shafa, entry, k)[-3:-1]:
            out.append((b["name"], b["fmt"], b["x"]))
    return out


def test_the_model_is_no_other_order_on_the_inputs_used(shafa):
    T = shafa.PLANES_TILE
    used = _used_inputs(shafa)
    assert {(f, x.size) for _, f, x in used} >= {(f, 513 * T + 5) for f in FMTS} | {(f, 2 * T + 3) for f in FMTS if f != "float16"}
    assert {f for _, f, x in used if 2 * T <= x.size < 256 * T} == set(FMTS)
    down_shows = set()
    for what, fmt, xb in used:
        term, fin = _terms(xb, fmt)
        model = gw.exact_sum(term, fin, T)
        seq, down, first = _other_orders(term, fin, T)
        assert model != seq, (what, fmt)
        if model != down:
            down_shows.add(q.ELEM[fmt])
        if xb.size > 256 * T:
            assert model != first, (what, fmt)
        else:
            assert model == first
    # a block's word is one rounding on top of its partials', so another tree shows in some blocks only: in one at least of
    # every element size here, and the GPU tests compare many more blocks than these
    assert down_shows == {2, 4, 8}


def _fused_lanes(a, b, fin, T):
    """the lanes of the first tile whose sum of a b changes when the product is contracted into the sum (exact rational
    arithmetic, one rounding a step) -> how many of the 256"""
    a, b, fin = a.tolist(), b.tolist(), fin.tolist()
    changed = 0
    for lane in range(256):
        s = f = 0.0
        for u in range(T // 4096):
            for i in range(16):
                j = u * 4096 + lane * 16 + i
                if j < len(a) and fin[j]:
                    s = s + a[j] * b[j]
                    f = float(Fraction(a[j]) * Fraction(b[j]) + Fraction(f))
        changed += s != f
    return changed


def _e_and_x(entry, b, fmt):
    xb = b["x"]
    if entry == "pair":
        yb = b["y"]
    elif entry == "round":
        yb = q._round(xb, q.MANT[fmt], b["keep"])[0]
    else:
        yb = q._quant(xb, b["step"], b["bound"])[0]
    x, y = q._dbl(xb, fmt), q._dbl(yb, fmt)
    with np.errstate(all="ignore"):
        return np.abs(x - y), x, np.isfinite(x) & np.isfinite(y)


def test_contraction_is_pinned_at_float64_and_only_there(shafa):
    """at float64 every entry has a block whose se2 and a block whose sx2 changes under contraction; at two and four bytes every
    product is exact, so contracting changes no bit"""
    T = shafa.PLANES_TILE
    seen = set()
    for entry, k in gw.ENTRIES:
        changed_e = changed_x = 0
        for b in gw.error_run_blocks(shafa, entry, k) + gw.quality_blocks(shafa, entry, k):
            if b["x"].size < T or (k < 8 and (entry, b["fmt"]) in seen) or (k == 8 and changed_e > 8 and changed_x > 8):
                continue
            seen.add((entry, b["fmt"]))
            e, x, fin = _e_and_x(entry, b, b["fmt"])
            e, x, fin = e[:T], x[:T], fin[:T]
            if k == 8:
                changed_e, changed_x = max(changed_e, _fused_lanes(e, e, fin, T)), max(changed_x, _fused_lanes(x, x, fin, T))
            else:
                assert all(Fraction(v) * Fraction(v) == Fraction(v * v) for v in e[fin].tolist()), (entry, b["fmt"])
                assert all(Fraction(v) * Fraction(v) == Fraction(v * v) for v in x[fin].tolist()), (entry, b["fmt"])
        assert k < 8 or (changed_e > 8 and changed_x > 8), (entry, changed_e, changed_x)
    assert seen == {(e, f) for e, k in gw.ENTRIES for f in q.FMTS[k]}
    # the long float64 block of section B
    b = gw.long_blocks(shafa, "pair", 8)[-3]
    e, x, fin = _e_and_x("pair", b, "float64")
    assert _fused_lanes(x[:T], x[:T], fin[:T], T) > 8 and _fused_lanes(e[:T], e[:T], fin[:T], T) > 8


def test_word_5_plants_fall_on_the_other_side_of_a_contracted_bound(shafa):
    T = shafa.PLANES_TILE
    assert gw.REL_ODD * 2 ** 20 != int(gw.REL_ODD * 2 ** 20)               # no power of two, nor a short fraction
    plants = gw.over_plants()
    assert sum(p[2] for p in plants) == 6 and sum(p[3] for p in plants) == 2 and all(p[2] != p[3] for p in plants)
    for x, y, as_header, contracted in plants:
        e = abs(x - y)
        assert (e > gw.ABS_ODD + gw.REL_ODD * abs(x)) == as_header
        assert (Fraction(e) > Fraction(gw.fused_bound(gw.ABS_ODD, gw.REL_ODD, x))) == contracted
    blks, plants = gw.overflow_blocks(shafa)
    w = [gw._want("pair", b, T)[1] for b in blks]
    assert w[0][7] == gw.INF_BITS and w[0][1] == 2 * T + 3 and w[0][9] != q.NONE
    assert w[1][6] == w[1][7] == w[1][8] == gw.INF_BITS and w[1][9] == 4321 and w[1][2] == 0 and w[1][5] == 1
    assert w[2][5] == 6 and w[2][2] == 0


# ---------------------------------------------------------------- D. the alignment tables
def test_error_alignment_table(shafa):
    T = shafa.PLANES_TILE
    for entry, k in gw.ENTRIES:
        blks = gw.error_align_blocks(shafa, entry, k)
        assert len(blks) == 19 * (16 // k)
        gw.assert_error_aligns(blks, k, T)
        assert {eal.own(b["a"] * k)[0] for b in blks} == {eal.own(A)[0] for A in range(0, 16, k)}      # every instantiation Q of err_tile
        key = {"round": lambda b: b["keep"], "quant": lambda b: b["step"], "pair": lambda b: (b["abs"], b["rel"])}[entry]
        assert len({key(b) for b in blks}) >= 4
        for thin in (blks[1:], blks[:-1], [b for b in blks if b["a"] != 2 % (16 // k)]):
            with pytest.raises(AssertionError):
                gw.assert_error_aligns(thin, k, T)


@pytest.mark.parametrize("k", (2, 4, 8))
def test_rounding_alignment_table(shafa, k):
    T = shafa.PLANES_TILE
    blocks, n_small = gw.round_align_blocks(shafa, k)
    assert n_small == 32 * (16 // k) and len(blocks) == n_small + (16 // k) * 5 * 23
    addr = [b[2] * k for b in blocks]
    gw.assert_round_classes(addr, blocks, n_small, k, T, cut=True)
    kinds = {(b[3], b[4]) for b in blocks}
    assert kinds == {(f, kp) for f in q.FMTS[k] for kp in (0, 1, q.MANT[f] // 2, q.MANT[f] - 1, q.MANT[f])}
    for a in eal.aligns(k):                                                # at every alignment every format and kept width
        assert {(b[3], b[4]) for b in blocks if b[2] == a} == kinds, (k, a)
    # thinned: without the small table the heads are not all there, without an alignment the pairs are not
    with pytest.raises(AssertionError):
        gw.assert_round_classes(addr[n_small // 2:], blocks[n_small // 2:], n_small // 2, k, T)
    keep = [i for i, b in enumerate(blocks) if b[2] != 16 // k - 1]
    with pytest.raises(AssertionError):
        gw.assert_round_classes([addr[i] for i in keep], [blocks[i] for i in keep], sum(i < n_small for i in keep), k, T, cut=True)
    big = [b for b in blocks[n_small:] if b[0] > 17]
    with pytest.raises(AssertionError):
        eal._assert_cut_words([b[2] * k for b in big], [b[:3] for b in big], k, T)
