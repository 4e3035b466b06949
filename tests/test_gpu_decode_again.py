"""A block decoded again, through every single-set decode driver.

sf_decode_dev has one slot for a table with 33..64-bit codes: of the blocks of one call that need it, all but one come back
LACK_OF_MEMORY and are decoded again on their own, and whatever reads the decoded regions (the pack, compare_dev,
crc32_dev, find_dev, seek_index_dev) is enqueued a second time for the same group.  A reader must then leave what a single
call would have left: nothing compared, digested or counted twice.

One mode-N .shaf + .cod of three blocks whose tables all hold a code above 32 bits (the construction of
tests/test_gpu_unpack_files.py::test_long_codes_in_several_files), at max_bytes=1 (a group per block: decompress_files and
decompress_range still decode several blocks in one call) and at the default (one group of three).  The references are the
host's: the concatenated blocks, zlib.crc32, bytes.find."""
import zlib

import numpy as np
import pytest

from test_gpu_pack import _cod_text
from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import _bytes, _cod_file, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def long_set(oracle, shafa):
    """(the blocks' bytes, the file arguments)"""
    from test_gpu_parity import long_code_case, to_shafa_table
    blocks, texts, pays = [], [], []
    for b in range(3):
        otab, data = long_code_case(oracle, 20000 + 1000 * b, 60 - 3 * b, 0.5, 30 + b)
        tab = to_shafa_table(shafa, otab)
        assert max(bytes(tab.len)) > 32
        blocks.append(data.tobytes())
        texts.append(_cod_text(shafa, tab))
        pays.append(shafa.sf_encode(data, tab).tobytes())
    cod = _cod_file(b"N", [len(d) for d in blocks], texts)
    shaf = b"@3" + b"".join(b"@" + str(len(p)).encode() + b"@" + p for p in pays)
    return blocks, dict(shaf=_t(shaf, 3), cod=_t(cod, 6))


def _occurrences(data, pat):
    out, i = [], data.find(pat)
    while i >= 0:
        out.append(i)
        i = data.find(pat, i + 1)
    return out


@pytest.mark.parametrize("mb", [1, None], ids=["max_bytes=1", "default"])
def test_every_reader_after_a_block_decoded_again(shafa, monkeypatch, long_set, mb):
    blocks, kw = long_set
    want = b"".join(blocks)
    n = len(want)
    seam = len(blocks[0]) + len(blocks[1])
    sf = _count_calls(shafa, monkeypatch, "sf_decode_dev")

    def again(one_call_decodes_several=True):
        """the path was taken: sf_decode_dev ran more than once, and where one call held several blocks, once on one alone"""
        calls = [len(a[2]) for a in sf]
        sf.clear()
        assert len(calls) > 1, calls
        if one_call_decodes_several:
            assert max(calls) > 1 and 1 in calls, calls

    assert _bytes(shafa.decompress_files(decode_rle=False, max_bytes=mb, **kw)) == want
    again()

    lo, hi = seam - 300, seam + 500
    assert _bytes(shafa.decompress_range(lo, hi - lo, max_bytes=mb, **kw)) == want[lo:hi]
    again()

    assert shafa.verify_files(_t(want, 1), decode_rle=False, max_bytes=mb, **kw) == shafa.Verify(True, None, n)
    again(mb is None)
    at = seam + 777
    flipped = want[:at] + bytes([want[at] ^ 0x20]) + want[at + 1:]
    assert shafa.verify_files(_t(flipped, 1), decode_rle=False, max_bytes=mb, **kw) == shafa.Verify(False, at, n)
    again(mb is None)

    assert shafa.checksum_files(decode_rle=False, max_bytes=mb, **kw) == shafa.Checksum(zlib.crc32(want), n)
    again(mb is None)

    pat2 = blocks[0][:2]
    assert all(pat2 in b for b in blocks)
    common = bytes([int(np.bincount(np.frombuffer(want, dtype=np.uint8)).argmax())])
    for pat, max_hits in ((pat2, 65536), (common, 5)):
        occ = _occurrences(want, pat)
        assert len(occ) > max(3, min(max_hits, 5))
        got = shafa.find_files(pat, decode_rle=False, max_hits=max_hits, max_bytes=mb, **kw)
        assert (got.count, got.positions.tolist(), got.size) == (len(occ), occ[:max_hits], n), (pat, got.count, len(occ))
        again(mb is None)

    index = shafa.build_index(span=256, max_bytes=mb, **kw)
    again(mb is None)
    assert [k.indexed for k in index.blocks] == [False] * 3
    assert [k.decoded_size for k in index.blocks] == [len(b) for b in blocks] and index.decoded_size == n
    ranges = [(len(blocks[0]) - 100, 300), (seam + 5, 1000)]
    out, offsets = shafa.read_ranges(index, ranges, **kw)
    assert offsets == [0, 300, 1300]
    assert _bytes(out) == b"".join(want[o:o + k] for o, k in ranges)
