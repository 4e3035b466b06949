"""Module C from device-resident tables and block sizes (shafa_hipd_sf_encode_dev, csrc/sf_encode_dev.hip).

Every case runs the host-table entry point (shafa_hipd_sf_encode, or _tiles with the tile histograms) on the same data in
the same process and requires the same bytes, sizes and per-block codes from sf_encode_dev; the cases whose tables come
from Module T on the device are also checked against the oracle (orc.sf_encode).  Guard bytes behind every output region
must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import long_code_case, to_shafa_table

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def layout(sizes, align=16, pad=0):
    off, pos = [], 0
    for n in sizes:
        off.append(pos)
        pos += (n + align - 1) // align * align + pad
    return off, max(pos, 16)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _upload(blocks, caps):
    import torch
    off, pos = layout(caps)
    host = np.zeros(pos, dtype=np.uint8)
    for o, b in zip(off, blocks):
        host[o:o + b.size] = b
    return off, torch.from_numpy(host).to(_dev())


def _tables_dev(tables):
    import torch
    tsz = C.sizeof(C.c_uint8) * (256 + 256 * 32)
    raw = np.zeros(len(tables) * tsz, dtype=np.uint8)
    for i, t in enumerate(tables):
        raw[i * tsz:(i + 1) * tsz] = np.frombuffer(bytes(t), dtype=np.uint8)
    return torch.from_numpy(raw).to(_dev())


def _tile_hists(shafa, bt, st, d_in, off, sizes, caps):
    import torch
    toff, tpos = layout([shafa.tile_hist_bytes(c) for c in caps])
    d_th = torch.zeros(tpos + 16, dtype=torch.uint8, device=_dev())
    d_freq = torch.zeros(len(sizes) * 256, dtype=torch.int64, device=_dev())
    bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
    return d_th, toff, d_freq


def encode_both(shafa, bt, st, d_in, off, in_cap, sizes, tables, out_cap, d_tab=None, d_in_n=None, thist=None,
                dev_sizes=None):
    """Host-table entry and sf_encode_dev on the same inputs.  Returns ((codes, sizes, outputs) host, (...) dev); outputs
    include the guard bytes behind each region."""
    import torch
    nb = len(sizes)
    ooff, opos = layout(out_cap, pad=GUARD)
    res = []
    for which in ("host", "dev"):
        d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
        d_n = torch.full((nb,), -1, dtype=torch.int64, device=_dev())
        if which == "host":
            if thist is None:
                bt.sf_encode(st, d_in, off, sizes, tables, d_out, ooff, out_cap, d_n)
            else:
                bt.sf_encode_tiles(st, d_in, off, sizes, tables, thist[0], thist[1], d_out, ooff, out_cap, d_n)
        else:
            tab = d_tab if d_tab is not None else _tables_dev(tables)
            nn = d_in_n if d_in_n is not None else torch.tensor(
                dev_sizes if dev_sizes is not None else sizes, dtype=torch.int64).to(_dev())
            bt.sf_encode_dev(st, d_in, off, in_cap, nn, tab, d_out, ooff, out_cap, d_n,
                             *(thist if thist is not None else (None, None)))
        _, errs = bt.finish(st, nb, raise_on_error=False)
        out = d_out.cpu().numpy()
        regions = [out[o:o + ((c + 15) // 16 * 16) + GUARD] for o, c in zip(ooff, out_cap)]
        res.append((errs, [int(x) for x in d_n.cpu().numpy()], regions))
    return res[0], res[1]


def check_same(host, dev, out_cap, what=""):
    herr, hn, hout = host
    derr, dn, dout = dev
    assert derr == herr, f"{what}: per-block codes differ: host {herr} dev {derr}"
    for b, cap in enumerate(out_cap):
        region = dout[b]
        assert (region[cap:] == FILL).all(), f"{what}: block {b} wrote past its output region"
        if herr[b] == 0:
            assert dn[b] == hn[b], f"{what}: block {b} size {dn[b]} != host {hn[b]}"
            assert region[:dn[b]].tobytes() == hout[b][:hn[b]].tobytes(), f"{what}: block {b} bytes differ"


def _lmax(t):
    return max(bytes(t.len))


# ---- F -> T -> C on the device, nothing read back in between ---------------------------------------------------------
def _streams(oracle, shafa):
    synth = __import__("pkgload").load_submodule("synth")
    zt = shafa.zipf_table(1.2)
    return {
        "zipf": lambda n, s: oracle.gen_bytes(s, n, zt),
        "runs": lambda n, s: synth.runs_stream(s, n, zt),
        "text": lambda n, s: synth.text_stream(s, n),
        "binary": lambda n, s: synth.binary_stream(s, n),
        "uniform": lambda n, s: oracle.gen_bytes(s, n),
    }


def chain(shafa, oracle, blocks, rle, tiles):
    """F (hist256_tiles or rle_encode_tiles) -> T (sf_build_codes) -> C (sf_encode_dev) enqueued back to back; then the
    host-table entry on what F and T left, and the oracle."""
    import torch
    dev = _dev()
    st = torch.cuda.Stream(device=dev)
    nb = len(blocks)
    sizes = [b.size for b in blocks]
    off, d_in = _upload(blocks, sizes)
    tsz = C.sizeof(shafa.CodeTable)
    d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
    d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    if rle:
        ccap = [2 * n + 16 for n in sizes]
        coff, cpos = layout(ccap)
        d_c = torch.zeros(cpos, dtype=torch.uint8, device=dev)
        d_cn = torch.zeros(nb, dtype=torch.int64, device=dev)
    else:
        ccap, coff, d_c = sizes, off, d_in
        d_cn = torch.tensor(sizes, dtype=torch.int64).to(dev)
    toff, tpos = layout([shafa.tile_hist_bytes(c) for c in ccap])
    d_th = torch.zeros(tpos + 16, dtype=torch.uint8, device=dev)
    out_cap = [c + 16 if c == 0 else (c * 8 + 16 if c < (1 << 20) else c * 3 + 16) for c in ccap]   # large: Zipf codes < 24 bits
    ooff, opos = layout(out_cap, pad=GUARD)
    d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=dev)
    d_n = torch.full((nb,), -1, dtype=torch.int64, device=dev)
    bt = shafa.Batch(nb, max(max(ccap), 1))
    if rle:
        bt.rle_encode_tiles(st, d_in, off, sizes, d_c, coff, ccap, d_cn, d_freq, d_th, toff)
    else:
        bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
    bt.sf_build_codes(st, nb, d_freq, d_tab)
    bt.sf_encode_dev(st, d_c, coff, ccap, d_cn, d_tab, d_out, ooff, out_cap, d_n,
                     *((d_th, toff) if tiles else (None, None)))
    _, derr = bt.finish(st, nb, raise_on_error=False)
    out = d_out.cpu().numpy()
    dn = [int(x) for x in d_n.cpu().numpy()]
    cn = [int(x) for x in d_cn.cpu().numpy()]
    cdata = d_c.cpu().numpy()
    freq = d_freq.cpu().numpy().astype(np.uint64).reshape(nb, 256)
    tabs = [shafa.CodeTable.from_buffer_copy(d_tab[i * tsz:(i + 1) * tsz].cpu().numpy().tobytes()) for i in range(nb)]
    dev_res = (derr, dn, [out[o:o + ((c + 15) // 16 * 16) + GUARD] for o, c in zip(ooff, out_cap)])
    host_res, _ = encode_both(shafa, bt, st, d_c, coff, ccap, cn, tabs, out_cap,
                              thist=(d_th, toff) if tiles else None)
    check_same(host_res, dev_res, out_cap, f"chain rle={rle} tiles={tiles}")
    for i in range(nb):
        cb = cdata[coff[i]:coff[i] + cn[i]]
        ot = oracle.sf_build(freq[i])
        assert bytes(ot.len) == bytes(tabs[i].len) and bytes(ot.bits) == bytes(tabs[i].bits), f"block {i}: table"
        if _lmax(ot) == 0 or cn[i] == 0:
            assert dn[i] == 0 and derr[i] == 0
            continue
        rc, want = oracle.sf_encode(cb, ot)
        assert rc == 0 and derr[i] == 0, (i, rc, derr[i])
        assert dn[i] == want.size and dev_res[2][i][:dn[i]].tobytes() == want.tobytes(), f"block {i} differs from oracle"
    bt.close()


SMALL_SIZES = [0, 1, 15, 32767, 32768, 32769, 100000 + 7, 3 * 32768 + 4095]


@pytest.mark.parametrize("tiles", [False, True])
@pytest.mark.parametrize("rle", [False, True])
def test_chain_small_blocks(oracle, shafa, rle, tiles):
    gens = _streams(oracle, shafa)
    blocks = []
    for k, (name, g) in enumerate(gens.items()):
        for j, n in enumerate(SMALL_SIZES):
            blocks.append(np.ascontiguousarray(g(n, 1000 + 17 * k + j), dtype=np.uint8))
    chain(shafa, oracle, blocks, rle, tiles)


@pytest.mark.parametrize("tiles", [False, True])
def test_chain_large_blocks(oracle, shafa, tiles):
    zt = shafa.zipf_table(1.2)
    sizes = [8 << 20, (8 << 20) - 5, (8 << 20) + 12345, 64 << 20]
    blocks = [oracle.gen_bytes(300 + i, n, zt) for i, n in enumerate(sizes)]
    chain(shafa, oracle, blocks, False, tiles)


def test_chain_large_rle(oracle, shafa):
    synth = __import__("pkgload").load_submodule("synth")
    zt = shafa.zipf_table(1.2)
    blocks = [synth.runs_stream(400 + i, n, zt) for i, n in enumerate([8 << 20, (8 << 20) + 77])]
    chain(shafa, oracle, blocks, True, True)


@pytest.mark.parametrize("nb", [1, 2, 5, 6, 7, 80, 128])
@pytest.mark.parametrize("tiles", [False, True])
def test_block_counts(oracle, shafa, nb, tiles):
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(500 + i, 20000 + 3331 * (i % 7), zt) for i in range(nb)]
    chain(shafa, oracle, blocks, False, tiles)


# ---- hand-made device tables, every class in one launch ----------------------------------------------------------------
def handmade(oracle, shafa):
    """(blocks, tables, out_cap) mixing longest codes 8, <= 12, 13..16, 17..32, > 32, an empty table, a missing symbol,
    an overflow and both faults."""
    blocks, tabs, caps = [], [], []

    def add(data, tab, cap=None):
        blocks.append(np.ascontiguousarray(data, dtype=np.uint8))
        tabs.append(tab)
        caps.append(cap if cap is not None else data.size * max(_lmax(tab), 1) // 8 + 16)

    u = oracle.gen_bytes(7, 70000)
    add(u, to_shafa_table(shafa, oracle.sf_build(oracle.hist256(u))))                   # uniform bytes: 9 bits
    # longest codes 8, 10, 13, 15, 16, 23, 52
    for nsyms, n, seed in ((9, 30000, 6), (11, 50000, 1), (14, 90001, 2), (16, 33000, 3), (17, 65536 + 9, 7), (24, 120000, 4),
                           (60, 70001, 5)):
        ot, data = long_code_case(oracle, n, nsyms, 0.5, seed)
        add(data, to_shafa_table(shafa, ot))
    add(oracle.gen_bytes(9, 5000), shafa.CodeTable())                                   # empty table
    zt = shafa.zipf_table(1.2)
    z = oracle.gen_bytes(11, 40000, zt)
    t = to_shafa_table(shafa, oracle.sf_build(oracle.hist256(z)))
    missing = shafa.CodeTable.from_buffer_copy(bytes(t))
    missing.len[int(z[100])] = 0                                                         # a symbol the data holds
    add(z, missing)
    add(z, t, cap=1000)                                                                  # output does not fit
    add(z, missing, cap=1000)                                                            # both faults
    add(np.zeros(0, dtype=np.uint8), t)                                                  # empty block
    lm = sorted(_lmax(t) for t in tabs)
    assert 8 in lm and 16 in lm and any(9 <= x <= 12 for x in lm) and any(13 <= x <= 15 for x in lm)
    assert any(17 <= x <= 32 for x in lm) and any(x > 32 for x in lm), lm
    return blocks, tabs, caps


def _run_handmade(oracle, shafa, tiles, blocks=None, tabs=None, caps=None, expect=None):
    import torch
    if blocks is None:
        blocks, tabs, caps = handmade(oracle, shafa)
    st = torch.cuda.Stream(device=_dev())
    sizes = [b.size for b in blocks]
    off, d_in = _upload(blocks, sizes)
    bt = shafa.Batch(len(blocks), max(sizes))
    th = None
    if tiles:
        d_th, toff, _ = _tile_hists(shafa, bt, st, d_in, off, sizes, sizes)
        bt.finish(st, len(blocks))
        th = (d_th, toff)
    host, dev = encode_both(shafa, bt, st, d_in, off, sizes, sizes, tabs, caps, thist=th)
    check_same(host, dev, caps, f"handmade tiles={tiles}")
    if expect is not None:
        assert dev[0] == expect(len(blocks)), dev[0]
    bt.close()
    return dev


@pytest.mark.parametrize("tiles", [False, True])
def test_handmade_tables_mixed(oracle, shafa, tiles):
    dev = _run_handmade(oracle, shafa, tiles)
    errs = dev[0]
    assert errs[:9] == [0] * 9
    assert errs[9:] == [shafa.FILE_UNRECOGNIZABLE, shafa.LACK_OF_MEMORY, shafa.FILE_UNRECOGNIZABLE, 0], errs
    assert dev[1][8] == 0 and dev[1][12] == 0                                            # empty table, empty block


@pytest.mark.parametrize("tiles", [False, True])
def test_several_generic_blocks(oracle, shafa, tiles):
    """Blocks of codes longer than 32 bits, of different sizes, among blocks of the other classes in one launch: the
    generic kernel's compacted list and its loop over blocks x tiles."""
    zt = shafa.zipf_table(1.2)
    blocks, tabs, caps = [], [], []
    for i, (nsyms, n) in enumerate(((60, 70001), (0, 50000), (40, 41), (0, 300000), (50, 5000), (45, 262144 + 3), (0, 1024))):
        if nsyms:
            ot, data = long_code_case(oracle, n, nsyms, 0.5, 40 + i)
        else:
            data = oracle.gen_bytes(40 + i, n, zt)
            ot = oracle.sf_build(oracle.hist256(data))
        blocks.append(np.ascontiguousarray(data, dtype=np.uint8))
        tabs.append(to_shafa_table(shafa, ot))
        caps.append(data.size * max(_lmax(tabs[-1]), 1) // 8 + 16)
    assert sum(_lmax(t) > 32 for t in tabs) == 4
    dev = _run_handmade(oracle, shafa, tiles, blocks, tabs, caps)
    assert dev[0] == [0] * len(blocks)


def test_foreign_tile_histograms(oracle, shafa):
    import torch
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(600 + i, 100000 + i, zt) for i in range(3)]
    tabs = [to_shafa_table(shafa, oracle.sf_build(oracle.hist256(b))) for b in blocks]
    sizes = [b.size for b in blocks]
    caps = [n * 2 + 16 for n in sizes]
    st = torch.cuda.Stream(device=_dev())
    off, d_in = _upload(blocks, sizes)
    bt = shafa.Batch(3, max(sizes))
    d_th, toff, _ = _tile_hists(shafa, bt, st, d_in, off, sizes, sizes)
    bt.finish(st, 3)
    d_th[toff[1]:toff[1] + 512] = 0x11                                                 # block 1's first tile: foreign
    host, dev = encode_both(shafa, bt, st, d_in, off, sizes, sizes, tabs, caps, thist=(d_th, toff))
    check_same(host, dev, caps, "foreign tile histograms")
    assert dev[0] == [0, shafa.OUTSIDE_MODULE, 0], dev[0]
    bt.close()


@pytest.mark.parametrize("tiles", [False, True])
def test_size_past_capacity(oracle, shafa, tiles):
    """d_in_n[b] > h_in_cap[b]: SHAFA_OUTSIDE_MODULE for that block only, size 0, nothing written."""
    import torch
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(700 + i, 50000, zt) for i in range(4)]
    tabs = [to_shafa_table(shafa, oracle.sf_build(oracle.hist256(b))) for b in blocks]
    sizes = [b.size for b in blocks]
    caps = [n * 2 + 16 for n in sizes]
    st = torch.cuda.Stream(device=_dev())
    off, d_in = _upload(blocks, [n + 64 for n in sizes])
    bt = shafa.Batch(4, max(sizes) + 64)
    th = None
    if tiles:
        d_th, toff, _ = _tile_hists(shafa, bt, st, d_in, off, sizes, [n + 64 for n in sizes])
        bt.finish(st, 4)
        th = (d_th, toff)
    dev_sizes = list(sizes)
    dev_sizes[2] = sizes[2] + 1
    host, dev = encode_both(shafa, bt, st, d_in, off, sizes, sizes, tabs, caps, thist=th, dev_sizes=dev_sizes)
    assert dev[0] == [0, 0, shafa.OUTSIDE_MODULE, 0], dev[0]
    assert dev[1][2] == 0 and (dev[2][2] == FILL).all()
    for b in (0, 1, 3):
        assert dev[1][b] == host[1][b] and dev[2][b][:dev[1][b]].tobytes() == host[2][b][:host[1][b]].tobytes()
    bt.close()


@pytest.mark.parametrize("knob,value", [("sf_encode_lanes", 256), ("sf_encode_lanes", 512), ("sf_encode_window_bits", 4),
                                        ("sf_encode_one_pass_min_blocks", 1), ("sf_encode_one_pass_min_blocks", 1000)])
@pytest.mark.parametrize("tiles", [False, True])
def test_knobs(oracle, shafa, knob, value, tiles):
    zt = shafa.zipf_table(1.2)
    blocks, tabs, caps = handmade(oracle, shafa)
    for i in range(8):                                                                    # enough blocks for the one-pass forms
        b = oracle.gen_bytes(800 + i, 200000 + 8191 * i, zt)
        blocks.append(b)
        tabs.append(to_shafa_table(shafa, oracle.sf_build(oracle.hist256(b))))
        caps.append(b.size * 2 + 16)
    shafa.set_option(knob, value)
    try:
        _run_handmade(oracle, shafa, tiles, blocks, tabs, caps)
    finally:
        shafa.set_option(knob, 0)


def test_no_synchronisation_inside_the_call(oracle, shafa):
    """With a long piece of GPU work in front of it on the stream, F -> T -> C enqueues and returns while the stream is
    still busy; one synchronisation at the end, then the bytes are checked."""
    import torch
    dev = _dev()
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(900 + i, 1 << 20, zt) for i in range(4)]
    sizes = [b.size for b in blocks]
    nb = len(blocks)
    off, d_in = _upload(blocks, sizes)
    d_n_in = torch.tensor(sizes, dtype=torch.int64).to(dev)
    tsz = C.sizeof(shafa.CodeTable)
    d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
    d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    toff, tpos = layout([shafa.tile_hist_bytes(n) for n in sizes])
    d_th = torch.zeros(tpos, dtype=torch.uint8, device=dev)
    caps = [n * 2 + 16 for n in sizes]
    ooff, opos = layout(caps)
    d_out = torch.zeros(opos, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(nb, max(sizes))

    def enqueue():
        bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
        bt.sf_build_codes(st, nb, d_freq, d_tab)
        bt.sf_encode_dev(st, d_in, off, sizes, d_n_in, d_tab, d_out, ooff, caps, d_n, d_th, toff)

    enqueue()                                                                             # warm-up: the batch grows here
    bt.finish(st, nb)
    d_out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)                                                    # ~0.1 s of one busy wave
    enqueue()
    busy = not st.query()
    bt.finish(st, nb)
    assert busy, "the stream had drained when the calls returned: something synchronised"
    out = d_out.cpu().numpy()
    for i, b in enumerate(blocks):
        rc, want = oracle.sf_encode(b, oracle.sf_build(oracle.hist256(b)))
        assert rc == 0 and int(d_n[i]) == want.size and out[ooff[i]:ooff[i] + want.size].tobytes() == want.tobytes()
    bt.close()
