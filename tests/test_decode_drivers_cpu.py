"""The parse rules of the decode drivers, as the one host function both the single-set drivers and decompress_many call
(DESIGN.md 7.27): one file's info words, per-block error codes, payload sizes and symbol counts as plain lists, `sf` and
the accepted modes -> (mode, fb, perr), or the ShafaError the drivers raise.  Cases written out; no device."""
import pytest

OK = 0


def _info(shafa, mode, count, indexed, status=0):
    w = [0] * shafa.UNPACK_INFO_WORDS
    w[shafa.INFO_STATUS], w[shafa.INFO_MODE], w[shafa.INFO_COUNT], w[shafa.INFO_INDEXED] = status, ord(mode), count, indexed
    return w


def _rules(shafa, info, errs, pn, nsym, sf, modes):
    return shafa._parse_rules("drv", info, errs, pn, nsym, sf, modes)


def _raises(shafa, code, text, *a):
    with pytest.raises(shafa.ShafaError) as e:
        _rules(shafa, *a)
    assert e.value.code == code and text in str(e.value), e.value


@pytest.mark.parametrize("modes", ["R", "RN"])
@pytest.mark.parametrize("sf", [True, False])
def test_header_and_mode(shafa, sf, modes):
    nsym = [100, 100] if sf else None
    # a bad header comes before everything else, whatever the other words hold
    _raises(shafa, shafa.FILE_STREAM_FAILED, "drv: bad header", _info(shafa, "N", 2, 2, status=1), [OK, OK], [50, 50], nsym, sf,
            modes)
    _raises(shafa, shafa.FILE_STREAM_FAILED, "drv: bad header", _info(shafa, "R", 2, 2, status=3), [7, OK], [50, 50], nsym, sf,
            modes)
    # mode R is accepted by both values; mode N only where it is named; another letter nowhere
    assert _rules(shafa, _info(shafa, "R", 2, 2), [OK, OK], [50, 50], nsym, sf, modes) == ("R", 2, OK)
    if "N" in modes:
        assert _rules(shafa, _info(shafa, "N", 2, 2), [OK, OK], [50, 50], nsym, sf, modes) == ("N", 2, OK)
    else:
        _raises(shafa, shafa.FILE_UNRECOGNIZABLE, "drv: mode 'N'", _info(shafa, "N", 2, 2), [OK, OK], [50, 50], nsym, sf, modes)
    _raises(shafa, shafa.FILE_UNRECOGNIZABLE, "drv: mode 'X'", _info(shafa, "X", 2, 2), [OK, OK], [50, 50], nsym, sf, modes)
    # the mode rule comes before a parse fault on block 0
    _raises(shafa, shafa.FILE_UNRECOGNIZABLE, "drv: mode 'X'", _info(shafa, "X", 2, 2), [shafa.FILE_STREAM_FAILED, OK], [50, 50],
            nsym, sf, modes)


@pytest.mark.parametrize("modes", ["R", "RN"])
@pytest.mark.parametrize("sf", [True, False])
def test_parse_faults(shafa, sf, modes):
    four = [100, 200, 300, 400]
    nsym = [150, 250, 350, 450] if sf else None
    for code in (shafa.FILE_STREAM_FAILED, shafa.FILE_UNRECOGNIZABLE, shafa.LACK_OF_MEMORY):
        # at block 0: raised, that code
        _raises(shafa, code, "drv: block 0", _info(shafa, "R", 4, 4), [code, OK, OK, OK], four, nsym, sf, modes)
        # at block 2 of 4: the blocks in front stay, the fault is the caller's to raise where its sequence says
        assert _rules(shafa, _info(shafa, "R", 4, 4), [OK, OK, code, OK], four, nsym, sf, modes) == ("R", 2, code)
        # the first fault in block order
        assert _rules(shafa, _info(shafa, "R", 4, 4), [OK, code, OK, shafa.FILE_INACCESSIBLE], four, nsym, sf, modes) == \
            ("R", 1, code)
    # error words behind the indexed blocks are not this file's
    assert _rules(shafa, _info(shafa, "R", 2, 2), [OK, OK, 9, 9], four, nsym, sf, modes) == ("R", 2, OK)
    # more blocks announced than indexed, no fault: FILE_STREAM_FAILED at the first block not indexed
    assert _rules(shafa, _info(shafa, "R", 6, 4), [OK] * 4, four, nsym, sf, modes) == ("R", 4, shafa.FILE_STREAM_FAILED)
    # ... but a fault among the indexed ones comes first
    assert _rules(shafa, _info(shafa, "R", 6, 4), [OK, OK, OK, shafa.FILE_UNRECOGNIZABLE], four, nsym, sf, modes) == \
        ("R", 3, shafa.FILE_UNRECOGNIZABLE)
    # announced above indexed with nothing indexed: block 0
    _raises(shafa, shafa.FILE_STREAM_FAILED, "drv: block 0", _info(shafa, "R", 1, 0), [], [], [] if sf else None, sf, modes)
    # the empty file
    assert _rules(shafa, _info(shafa, "R", 0, 0), [], [], [] if sf else None, sf, modes) == ("R", 0, OK)
    assert _rules(shafa, _info(shafa, "R", 0, 0), [9, 9], [5, 5], [5, 5] if sf else None, sf, modes) == ("R", 0, OK)


@pytest.mark.parametrize("modes", ["R", "RN"])
def test_symbol_count_above_eight_a_payload_byte(shafa, modes):
    pn = [100, 37, 100]
    # 8 x pn symbols can be there (every code has >= 1 bit); one more cannot
    assert _rules(shafa, _info(shafa, "R", 3, 3), [OK] * 3, pn, [800, 8 * 37, 1], True, modes) == ("R", 3, OK)
    assert _rules(shafa, _info(shafa, "R", 3, 3), [OK] * 3, pn, [800, 8 * 37 + 1, 1], True, modes) == \
        ("R", 1, shafa.FILE_UNRECOGNIZABLE)
    _raises(shafa, shafa.FILE_UNRECOGNIZABLE, "drv: block 0", _info(shafa, "R", 3, 3), [OK] * 3, pn, [801, 1, 1], True, modes)
    # a parse fault of the block keeps its own code, and an earlier one comes first
    assert _rules(shafa, _info(shafa, "R", 3, 3), [OK, shafa.FILE_STREAM_FAILED, OK], pn, [1, 8 * 37 + 1, 1], True, modes) == \
        ("R", 1, shafa.FILE_STREAM_FAILED)
    assert _rules(shafa, _info(shafa, "R", 3, 3), [OK, shafa.FILE_STREAM_FAILED, OK], pn, [1, 1, 801], True, modes) == \
        ("R", 1, shafa.FILE_STREAM_FAILED)
    # .rle + .freq has no symbol counts: the payload sizes alone say nothing
    assert _rules(shafa, _info(shafa, "R", 3, 3), [OK] * 3, pn, None, False, modes) == ("R", 3, OK)
