"""What tests/test_gpu_far_offsets.py and tests/test_gpu_long_regions.py lean on, checked without a device: the arena's arithmetic,
the torch references of the long regions against numpy and zlib at small sizes on the CPU, and the planted find data."""
import zlib

import numpy as np
import pytest
import torch

import test_gpu_far_offsets as far
import test_gpu_long_regions as lng
from test_planes_grid_hist_cpu import plane_histograms, z_of


def _sides(shift_sides=True):
    """the shapes of the far-offset cases and more: empty, one byte, around a tile, 2 MiB; input and output, exact and rounded"""
    sizes = [0, 1, 5, 15, 16, 17, 8191, 8192, 8193, 3 * 8192 + 5, 32769, 65613, 131226 + 16, 256 * 8192 + 1]
    return [far.Side("in", [np.zeros(n, np.uint8) for n in sizes], any_align=shift_sides),
            far.Side("out", sizes, out=True),
            far.Side("planes", sizes * 8, out=True, exact=True),
            far.Side("el", sizes, out=True, exact=True, any_align=shift_sides)]


@pytest.mark.parametrize("shift", far.SHIFTS)
def test_arena_layouts(shift):
    sides = _sides()
    names = [s.name for s in sides]
    for far_set in [set(), set(names)] + [{n} for n in names]:
        lay = far.place(sides, far_set, shift)
        far.check_layout(lay)
        for s in sides:
            for o, n, room in lay[s.name]:
                assert (o >= far.G) == (s.name in far_set)
                assert o % 16 == (shift if s.any_align else 0)
                assert room >= n
                if o >= far.G:                                             # both misreadings: the shadow, inside the arena, on no near region
                    for m in far.misreadings(o):
                        assert m == o - far.G and 0 <= m - far.GUARD and m + room + far.GUARD <= far.LOW
                        assert m - far.GUARD >= far.NEAR[1]


def _far_cases():
    """every far test with every value of its parameters but the option sets, which change no placement"""
    out = []
    for name, fn in sorted(vars(far).items()):
        if not name.startswith("test_") or not callable(fn):
            continue
        combos = [{}]
        for m in getattr(fn, "pytestmark", []):
            if m.name != "parametrize":
                continue
            names = [n.strip() for n in m.args[0].split(",")]
            values = [{}] if names == ["options"] else list(m.args[1])
            combos = [{**c, **dict(zip(names, v if len(names) > 1 else (v,)))} for c in combos for v in values]
        out += [(name, c) for c in combos]
    return out


FAR_CASES = _far_cases()


@pytest.mark.parametrize("name,kw", FAR_CASES, ids=[n + "-" + "-".join(str(v) for v in c.values()) for n, c in FAR_CASES])
def test_every_placement_of_the_far_tests(name, kw, shafa, oracle, monkeypatch):
    """each far test is run on an arena without a device: it builds its real sides, and every placement it asks for (near, far,
    each side alone, + 5 and + 11) goes through check_layout; for every far region both misreadings are its shadow"""
    import contextlib
    import inspect
    monkeypatch.setattr(far, "DEV", "cpu")                                  # the cases' small tensors (tables, counts)
    monkeypatch.setattr(far, "options_set", lambda shafa, options: contextlib.nullcontext())
    arena = far.DryArena()
    fn = getattr(far, name)
    given = dict(arena=arena, shafa=shafa, oracle=oracle, **kw)
    fn(**{p: given[p] for p in inspect.signature(fn).parameters})
    assert len(arena.layouts) >= 2 and any("far" in label for label, _ in arena.layouts)
    for label, lay in arena.layouts:
        for rows in lay.values():
            for o, n, room in rows:
                if o >= far.G:
                    assert far.misreadings(o) == (o - far.G, o - far.G) and far.SHADOW[0] <= o - far.G < far.SHADOW[1], (label, o)


def test_misreadings():
    assert far.misreadings(far.G + 5) == (5, 5)
    assert far.misreadings(far.G + (1 << 31) + 5) == ((1 << 31) + 5, 5 - (1 << 31))       # why bit 31 stays clear
    assert far.ARENA_BYTES == (1 << 32) + (512 << 20)


def test_a_case_that_does_not_fit_is_refused():
    with pytest.raises(AssertionError):
        far.place([far.Side("in", [np.zeros(1, np.uint8)]), far.Side("out", [129 << 20], out=True)], {"in"})


def test_long_region_positions_stay_inside_the_allocation():
    assert lng.LONG == (1 << 32) + 3 * 8192 + 5 and lng.LEAD >= 1 << 31
    for start in (lng.LEAD, lng.LEAD + 4, lng.LEAD + 5):
        for p in (0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, lng.LONG - 1, lng.LONG):
            assert 0 <= start + lng.sign_extended(p) < lng.ALLOC
            assert 0 <= start + (p & 0xFFFFFFFF) < lng.ALLOC
            assert 0 <= start + p <= lng.ALLOC - lng.GUARD
    assert lng.sign_extended((1 << 31) + 7) == 7 - (1 << 31) and lng.sign_extended((1 << 32) + 7) == 7


# ---------------------------------------------------------------- the references
def test_crc_combine_against_zlib():
    rng = np.random.default_rng(1)
    for la, lb in [(0, 0), (0, 5), (5, 0), (1, 1), (3, 8), (1000, 1), (4097, 65536), (77, 1 << 20)]:
        a, b = rng.integers(0, 256, la, dtype=np.uint8).tobytes(), rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
        assert lng.crc_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def test_crc_of_span_against_zlib():
    period = np.random.default_rng(2).integers(0, 256, 1237, dtype=np.uint8).tobytes()
    whole = period * 60
    for start, n in [(0, 0), (0, 1), (0, 1237), (0, 1238), (3, 1234), (3, 1235), (5, 40000), (1236, 2), (2000, 50001), (0, len(whole))]:
        assert lng.crc_of_span(period, start, n) == zlib.crc32(whole[start:start + n]), (start, n)


def test_fill_repeat():
    period = lng.random_period(3, 101, "cpu")
    for n in (0, 1, 100, 101, 102, 1000):
        region = torch.full((n + 2,), 7, dtype=torch.uint8)
        lng.fill_repeat(region[1:1 + n], period)
        assert bytes(region.numpy()) == b"\x07" + (bytes(period.numpy()) * 11)[:n] + b"\x07"


@pytest.mark.parametrize("k", [1, 3, 4])
def test_torch_planes_against_numpy(k):
    raw = np.random.default_rng(4 + k).integers(0, 256, 1001 * k, dtype=np.uint8)
    got = lng.torch_planes(torch.from_numpy(raw), k)
    assert np.array_equal(got.numpy(), raw.reshape(-1, k).T)               # test_gpu_planes._planes_of's statement


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "int64"])
def test_torch_grid_z_and_plane_hist_against_numpy(dtype):
    """against test_planes_grid_hist_cpu.z_of (test_planes_grid_cpu.grid_diff, folded) and plane_histograms"""
    U = {"int8": np.uint8, "int16": np.uint16, "int32": np.uint32, "int64": np.uint64}[dtype]
    rng = np.random.default_rng(5)
    for n, lags in [(1, (1,)), (50, (1, 3)), (1000, (3, 5, 15)), (1000, (1, 64, 700)), (1000, (1, 999, 1000)), (300, (7, 400, 900)),
                    (4099, (1, 17, 153))]:
        x = np.frombuffer(rng.integers(0, 256, n * U().itemsize, dtype=np.uint8).tobytes(), U).copy()
        if n > 2:
            x[1], x[2] = np.iinfo(U).max, 0                                # wraps both ways
        t = torch.from_numpy(x.view(dtype))
        z = lng.torch_grid_z(t, lags)
        assert np.array_equal(t.numpy().view(U), x)                        # x is only read
        assert np.array_equal(z.numpy().view(U), z_of(x.copy(), lags)), (n, lags)
        assert np.array_equal(lng.torch_plane_hist(z, chunk=97).numpy().astype(np.uint64), plane_histograms(x.copy(), lags)), (n, lags)


@pytest.mark.parametrize("where", sorted(lng.PLANTED))
def test_planted_data_holds_the_pattern_where_it_was_planted_only(where):
    """the long regions' positions with the border at 2^16 and the region's end at 1 MiB"""
    n, pat = 1 << 20, lng.PATTERN
    hits = lng.planted_at(65536, n)[where]
    region = torch.full((n + 32,), lng.FILL, dtype=torch.uint8)
    lng.plant(region[16:16 + n], pat, hits, 3)
    raw = bytes(region.numpy())
    assert raw[:16] == raw[-16:] == bytes([lng.FILL]) * 16
    raw = raw[16:16 + n]
    found, at = [], raw.find(pat)
    while at >= 0:
        found.append(at)
        at = raw.find(pat, at + 1)
    assert tuple(found) == hits
    assert raw.count(pat[:1]) == len(hits)                                 # the alphabet holds no first byte of the pattern
    assert len(set(raw)) > 200
