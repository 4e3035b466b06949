"""The sequence of Batch calls of every single-set decode driver, written out.

A set of four blocks (3 x 4096 + 33 bytes at 4096 a block: the last block has 33 bytes) in the four forms of
test_gpu_verify_files._sets, at max_bytes=1 (every block its own group) and at the default (one group).  Every public
method of shafa.Batch but close is wrapped by a recorder of (method, number of blocks); each driver's recording is compared
with a list in this file.  The lists were recorded from the drivers as they stood before they shared one walk (DESIGN.md
7.27) and are not derived from the code under test: the Batch calls and the finish counts of a driver may not change.

The number of blocks of a call: the length of its first list argument, else its first int argument (unpack_cod's
max_blocks, finish's count); crc32_combine_dev: the blocks combined."""
import inspect

import pytest

from test_gpu_verify_files import _sets

pytestmark = pytest.mark.gpu

N, BS = 3 * 4096 + 33, 4096
FORMS = ["N", "rle+freq", "R", "R as .rle"]


def _blocks(name, a):
    if name == "crc32_combine_dev":
        return sum(a[2])
    for x in a[1:]:
        if isinstance(x, (list, tuple)):
            return len(x)
    return next(x for x in a[1:] if isinstance(x, int) and not isinstance(x, bool))


def _record_batch(shafa, monkeypatch):
    calls = []

    def wrap(name, real):
        def wrapper(self, *a, **k):
            calls.append(f"{name}:{_blocks(name, a)}")
            return real(self, *a, **k)
        return wrapper

    for name, real in inspect.getmembers(shafa.Batch, inspect.isfunction):
        if not name.startswith("_") and name != "close":
            monkeypatch.setattr(shafa.Batch, name, wrap(name, real))
    return calls


def _drivers(shafa, d_in, kw, mb):
    """name -> the call, for one set; decoded_sizes, decompress_range and build_index follow the .cod's mode"""
    files = {k: v for k, v in kw.items() if k != "decode_rle"}
    pat = bytes(d_in[100:103].cpu().tolist())
    return {"decompress_files": lambda: shafa.decompress_files(max_bytes=mb, **kw),
            "decoded_sizes": lambda: shafa.decoded_sizes(**files),
            "decompress_range": lambda: shafa.decompress_range(2 * BS + 100, 50, max_bytes=mb, **files),
            "verify_files": lambda: shafa.verify_files(d_in, max_bytes=mb, **kw),
            "checksum_files": lambda: shafa.checksum_files(max_bytes=mb, **kw),
            "find_files": lambda: shafa.find_files(pat, max_hits=8, max_bytes=mb, **kw),
            "build_index": lambda: shafa.build_index(span=256, max_bytes=mb, **files)}


def record(shafa, monkeypatch, form, mb):
    """driver -> its Batch calls as one string, "method:blocks method:blocks ..." """
    name, d_in, kw = _sets(shafa, N, BS)[FORMS.index(form)]
    assert name == form
    calls = _record_batch(shafa, monkeypatch)
    out = {}
    for driver, call in _drivers(shafa, d_in, kw, mb).items():
        calls.clear()
        call()
        out[driver] = " ".join(calls)
    return out


def _chains(parse, finish, rows):
    """the rows with P (the parse's calls, its synchronisation included) and F (a synchronisation) spelt out"""
    return {k: v.replace("P", parse + " " + finish).replace("F", finish) for k, v in rows.items()}


SF1, SF4 = "unpack_payloads:1 sf_decode_dev:1 ", "unpack_payloads:4 sf_decode_dev:4 "
# the two RLE forms in front of their groups: the payloads (SF-decoded for mode R) and the size pass
MEASURE_RLE = "P unpack_payloads:4 rle_decoded_size_dev:4 F "
MEASURE_R = "P " + SF4 + "F rle_decoded_size_dev:4 F "
FIND_SEAM = "find_dev:2 find_dev:1 "          # a group behind the first: the seam's two regions, then its own blocks


def _plain(sf):
    """the drivers that walk SF-decoded blocks group by group, a synchronisation each"""
    if sf == SF1:
        return {"verify_files": "P " + (SF1 + "compare_dev:1 F ") * 4,
                "checksum_files": "P " + (SF1 + "crc32_dev:1 F ") * 3 + SF1 + "crc32_dev:1 crc32_combine_dev:4 F",
                "find_files": "P " + SF1 + "find_dev:1 F " + (SF1 + FIND_SEAM + "F ") * 3}
    return {"verify_files": "P " + SF4 + "compare_dev:4 F",
            "checksum_files": "P " + SF4 + "crc32_dev:4 crc32_combine_dev:4 F",
            "find_files": "P " + SF4 + "find_dev:4 F"}


def _rle(measure, groups):
    """the drivers behind the measure: the groups back to back, one synchronisation at the end"""
    if groups == 4:
        return {"decompress_files": measure + "rle_decode_dev:1 pack_payloads:1 " * 4 + "F",
                "verify_files": measure + "rle_decode_dev:1 compare_dev:1 " * 4 + "F",
                "checksum_files": measure + "rle_decode_dev:1 crc32_dev:1 " * 4 + "crc32_combine_dev:4 F",
                "find_files": measure + "rle_decode_dev:1 find_dev:1 " + ("rle_decode_dev:1 " + FIND_SEAM) * 3 + "F"}
    return {"decompress_files": measure + "rle_decode_dev:4 pack_payloads:4 F",
            "verify_files": measure + "rle_decode_dev:4 compare_dev:4 F",
            "checksum_files": measure + "rle_decode_dev:4 crc32_dev:4 crc32_combine_dev:4 F",
            "find_files": measure + "rle_decode_dev:4 find_dev:4 F"}


def _by_mode(measure):
    """the drivers that take no decode_rle, on an RLE form: the same at every max_bytes but build_index's groups"""
    return {"decoded_sizes": measure.rstrip(),
            "decompress_range": measure + "rle_decode_dev:1 pack_payloads:1 F"}


COD_N, COD_R, FREQ = "unpack_cod:32 unpack_shaf:32", "unpack_cod:24 unpack_shaf:24", "unpack_rle_freq:449"
N_ROWS = {"decompress_files": "P " + SF4 + "pack_payloads:4 F",
          "decoded_sizes": "P",
          "decompress_range": "P " + SF1 + "pack_payloads:1 F"}
INDEX_R1 = "P " + (SF1 + "F seek_index_dev:1 F ") * 4
INDEX_R4 = "P " + SF4 + "F seek_index_dev:4 F"
EXPECTED = {
    ("N", 1): _chains(COD_N, "finish:32", {**N_ROWS, **_plain(SF1), "build_index": "P " + (SF1 + "seek_index_dev:1 F ") * 4}),
    ("N", None): _chains(COD_N, "finish:32", {**N_ROWS, **_plain(SF4), "build_index": "P " + SF4 + "seek_index_dev:4 F"}),
    ("rle+freq", 1): _chains(FREQ, "finish:449", {**_by_mode(MEASURE_RLE), **_rle(MEASURE_RLE, 4),
                                                  "build_index": "P " + "unpack_payloads:1 seek_index_dev:1 F " * 4}),
    ("rle+freq", None): _chains(FREQ, "finish:449", {**_by_mode(MEASURE_RLE), **_rle(MEASURE_RLE, 1),
                                                     "build_index": "P unpack_payloads:4 seek_index_dev:4 F"}),
    ("R", 1): _chains(COD_R, "finish:24", {**_by_mode(MEASURE_R), **_rle(MEASURE_R, 4), "build_index": INDEX_R1}),
    ("R", None): _chains(COD_R, "finish:24", {**_by_mode(MEASURE_R), **_rle(MEASURE_R, 1), "build_index": INDEX_R4}),
    # the mode-R pair read as its .rle bytes: mode N's chains where decode_rle is an argument, mode R's where the .cod decides
    ("R as .rle", 1): _chains(COD_R, "finish:24", {**_by_mode(MEASURE_R), **_plain(SF1), "build_index": INDEX_R1,
                                                   "decompress_files": "P " + SF4 + "pack_payloads:4 F"}),
    ("R as .rle", None): _chains(COD_R, "finish:24", {**_by_mode(MEASURE_R), **_plain(SF4), "build_index": INDEX_R4,
                                                      "decompress_files": "P " + SF4 + "pack_payloads:4 F"}),
}


@pytest.mark.parametrize("mb", [1, None], ids=["max_bytes=1", "default"])
@pytest.mark.parametrize("form", FORMS)
def test_batch_calls_of_every_driver(shafa, monkeypatch, form, mb):
    got = record(shafa, monkeypatch, form, mb)
    want = EXPECTED[form, mb]
    assert sorted(got) == sorted(want)
    for driver in got:
        print(f"{form} max_bytes={mb} {driver}: {got[driver]}")
        assert got[driver].split() == want[driver].split(), (form, mb, driver)
