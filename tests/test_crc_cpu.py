"""CPU-side checks of the CRC-32 entries (shafa_hipd_crc32_dev, shafa_hipd_crc32_combine_dev, csrc/crc32.hip) and of
shafa.crc32_combine / crc32 / checksum_files: declared, exported, bound in Python, the ABI version unchanged, every argument
error refused before HIP is touched, the host statement of the combine rule against zlib, and the ValueErrors (no GPU needed).
The kernels' constants are built at compile time and tied to the rule by static_asserts in crc32.hip; what is checked here is
the same statement of the rule in Python (_crc_mul, _crc_x_pow) against zlib and against zlib's published powers of x."""
import ctypes as C
import os
import random
import zlib

import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_crc32_dev", "shafa_hipd_crc32_combine_dev")


def test_declared_exported_and_bound(shafa):
    decl = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in decl and hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("crc32_dev", "crc32_combine_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("crc32", "crc32_combine", "checksum_files"):
        assert callable(getattr(shafa, name, None)), name
    assert shafa.Checksum._fields == ("crc32", "decoded_size")


def _i32(*v):
    return (C.c_int * len(v))(*v)


def test_crc32_dev_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.odd, off=_u64(0, 5, (1 << 40) + 3), cap=_u64(5, 100, 70000), d_in_n=A.p, d_crc=A.p)
        a.update(kw)
        return L.shafa_hipd_crc32_dev(a["b"], None, a["nb"], a["d_in"], a["off"], a["cap"], a["d_in_n"], a["d_crc"])

    # every check passed (an odd address and odd 64-bit offsets are fine): HIP refuses the stand-in batch
    assert call() not in (shafa.SUCCESS, OM, LM)
    for k in ("b", "d_in", "d_in_n", "d_crc", "off", "cap"):
        assert call(**{k: None}) == OM, k
    assert call(nb=0) == shafa.SUCCESS and call(nb=-4) == shafa.SUCCESS
    assert call(nb=0, off=None, cap=None) == shafa.SUCCESS             # nothing to digest or look at
    assert call(nb=0x7F7F7F7F + 1) == LM                               # past max_blocks: refused before an array is read
    assert call(nb=0x7FFFFFFF) == LM
    assert call(b=None, nb=0) == OM                                    # a NULL batch comes before nblocks
    assert call(b=None, nb=0x7FFFFFFF) == OM
    # 2^31 tiles of 8 KiB or more in the capacities, in one block or in their sum; one tile fewer gets to HIP
    T = 8192
    assert call(cap=_u64(5, (1 << 31) * T, 7)) == LM
    assert call(cap=_u64(1 << 43, 1 << 43, (1 << 31) * T - (1 << 44))) == LM
    assert call(cap=_u64((1 << 64) - 1, 0, 0)) == LM
    assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0)) not in (shafa.SUCCESS, OM, LM)
    assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1)) == LM


def test_crc32_combine_dev_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY

    def call(**kw):
        a = dict(b=A.p, nf=3, first=_i32(0, 0, 7), count=_i32(3, 0, 300), d_crc=A.p, d_n=A.p, d_file_crc=A.p, d_file_n=A.p)
        a.update(kw)
        return L.shafa_hipd_crc32_combine_dev(a["b"], None, a["nf"], a["first"], a["count"], a["d_crc"], a["d_n"],
                                              a["d_file_crc"], a["d_file_n"])

    assert call() not in (shafa.SUCCESS, OM, LM)                       # HIP refuses the stand-in batch
    for k in ("b", "d_crc", "d_n", "d_file_crc", "d_file_n", "first", "count"):
        assert call(**{k: None}) == OM, k
    assert call(nf=0) == shafa.SUCCESS and call(nf=-1) == shafa.SUCCESS
    assert call(nf=0, first=None, count=None) == shafa.SUCCESS
    assert call(b=None, nf=0) == OM
    assert call(nf=0x7F7F7F7F + 1) == LM and call(nf=0x7FFFFFFF) == LM
    assert call(first=_i32(0, -1, 7)) == OM
    assert call(count=_i32(3, 0, -1)) == OM
    assert call(first=_i32(0, 0, 0x7FFFFFFF), count=_i32(3, 0, 1)) == OM
    assert call(first=_i32(0, 0, 0x7FFFFFFF), count=_i32(3, 0, 0)) not in (shafa.SUCCESS, OM, LM)


def test_rule_in_python(shafa):
    """the arithmetic the kernels' constants are built from, stated in Python: powers of x against zlib's published table
    (crc32.h: x2n_table), the inverse, and the order of x"""
    one, x = 0x80000000, 0x40000000
    x2n = [0x40000000, 0x20000000, 0x08000000, 0x00800000, 0x00008000, 0xedb88320, 0xb1e6b092, 0xa06a2517, 0xed627dae,
           0x88d14467, 0xd7bbfe6a, 0xec447f11, 0x8e7ea170, 0x6427800e, 0x4d47bae0, 0x09fe548f, 0x83852d0f, 0x30362f1a,
           0x7b5a9cc3, 0x31fec169, 0x9fec022a, 0x6c8dedc4, 0x15d6874d, 0x5fde7a4e, 0xbad90e37, 0x2e4e5eef, 0x4eaba214,
           0xa8a472c0, 0x429a969e, 0x148d302a, 0xc40ba6d0, 0xc4e22c3c]
    assert [shafa._crc_x_pow(1 << k) for k in range(32)] == x2n
    assert shafa._crc_x_pow(0) == one and shafa._crc_x_pow(1) == x
    assert shafa._crc_x_pow(0xFFFFFFFF) == one and shafa._crc_x_pow(1 << 32) == x       # the order of x divides 2^32 - 1
    for z in (1, 2, 4095, 4096, 8191):                                  # x^(-8 z), what takes a tile's pad off again
        inv = shafa._crc_x_pow(0xFFFFFFFF - 8 * z)
        assert shafa._crc_mul(inv, shafa._crc_x_pow(8 * z)) == one
    # raw(M 0^z) = raw(M) x^(8 z): the finished CRC of M followed by z zero bytes, un-conditioned, divided by x^(8 z)
    rng = random.Random(5)
    for n, z in ((1, 8191), (9, 8183), (8192 + 1, 8191), (70, 1)):
        m = rng.randbytes(n)
        cond = shafa._crc_mul(0xFFFFFFFF, shafa._crc_x_pow(8 * (n + z)))            # what init and final XOR add
        raw_padded = zlib.crc32(m + bytes(z)) ^ 0xFFFFFFFF ^ cond
        raw = shafa._crc_mul(raw_padded, shafa._crc_x_pow(0xFFFFFFFF - 8 * z))
        assert raw ^ shafa._crc_mul(0xFFFFFFFF, shafa._crc_x_pow(8 * n)) ^ 0xFFFFFFFF == zlib.crc32(m)


def test_crc32_combine_against_zlib(shafa):
    rng = random.Random(11)
    assert shafa.crc32_combine(0, 0, 0) == 0
    assert shafa.crc32_combine(zlib.crc32(b"1234"), zlib.crc32(b"56789"), 5) == 0xCBF43926
    for i in range(300):
        n = rng.choice((0, 1, 2, 31, 32, 33, 255, 4096, 70001))
        data = rng.randbytes(n)
        k = 0 if i % 7 == 0 else n if i % 7 == 1 else rng.randint(0, n)            # empty halves included
        a, b = data[:k], data[k:]
        got = shafa.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b))
        assert got == zlib.crc32(data), (n, k)
    with pytest.raises(ValueError):
        shafa.crc32_combine(1, 2, -1)


def test_crc32_combine_is_associative_above_2_32(shafa):
    rng = random.Random(13)
    comb = shafa.crc32_combine
    for _ in range(40):
        a, b, c = (rng.getrandbits(32) for _ in range(3))
        lb, lc = (rng.choice(((1 << 32) + rng.randint(0, 99), (1 << 33) + 5, (1 << 40) - 1, 0, 7)) for _ in range(2))
        assert comb(a, comb(b, c, lc), lb + lc) == comb(comb(a, b, lb), c, lc), (a, b, c, lb, lc)
    # a length of k (2^32 - 1) bytes is a multiple of x's order in bits as well: crc1 passes unchanged
    assert comb(0x12345678, 0, 0xFFFFFFFF) == 0x12345678
    # zeros behind a message, by the rule and by zlib (small enough to run)
    z = 1 << 20
    assert comb(zlib.crc32(b"abc"), zlib.crc32(bytes(z)), z) == zlib.crc32(b"abc" + bytes(z))


def test_drivers_refuse_bad_arguments(shafa):
    import torch
    cpu = torch.zeros(8, dtype=torch.uint8)
    for e in ({"shaf": cpu, "cod": cpu}, {"rle": cpu, "freq": cpu}, {"shaf": cpu}, {"cod": cpu, "rle": cpu, "freq": cpu}, {},
              {"shaf": cpu, "cod": cpu, "rle": cpu}, {"rle": cpu}):
        with pytest.raises(ValueError):
            shafa.checksum_files(**e)
    for bad in (cpu, None, b"abc"):
        with pytest.raises(ValueError):
            shafa.crc32(bad)
