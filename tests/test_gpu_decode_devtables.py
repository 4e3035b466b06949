"""Module D from device-resident tables, stream sizes and symbol counts (shafa_hipd_sf_decode_dev, csrc/sfd_dev.hpp) and
RLE decode from device-resident sizes (shafa_hipd_rle_decode_dev).

Every case runs the host-table entry point (shafa_hipd_sf_decode / _rle_decode) on the same data in the same process and
requires the same bytes and per-block codes from the device entry; round trips are also checked against the input.  Guard
bytes behind every output region must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import parse_blocks_text, parse_shaf
from test_gpu_encode_devtables import FILL, GUARD, _dev, _streams, _tables_dev, _upload, layout
from test_gpu_parity import long_code_case, rd, to_shafa_table

pytestmark = pytest.mark.gpu


def _i64(xs):
    import torch
    return torch.tensor([int(x) for x in xs], dtype=torch.int64).to(_dev())


def decode_both(shafa, bt, st, d_in, off, in_cap, in_n, tables, nsym, out_cap, dev_in_n=None, dev_nsym=None):
    """Host-table sf_decode and sf_decode_dev on the same inputs -> ((codes, regions) host, (codes, regions) dev)."""
    import torch
    nb = len(in_n)
    ooff, opos = layout(out_cap, pad=GUARD)
    res = []
    for which in ("host", "dev"):
        d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
        if which == "host":
            bt.sf_decode(st, d_in, off, in_n, tables, nsym, d_out, ooff)
        else:
            bt.sf_decode_dev(st, d_in, off, in_cap, _i64(dev_in_n if dev_in_n is not None else in_n), _tables_dev(tables),
                             _i64(dev_nsym if dev_nsym is not None else nsym), d_out, ooff, out_cap)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        out = d_out.cpu().numpy()
        res.append((errs, [out[o:o + ((c + 15) // 16 * 16) + GUARD] for o, c in zip(ooff, out_cap)]))
    return res[0], res[1]


def check_same(host, dev, nsym, out_cap, what=""):
    (herr, hout), (derr, dout) = host, dev
    assert derr == herr, f"{what}: per-block codes differ: host {herr} dev {derr}"
    for b, cap in enumerate(out_cap):
        assert (dout[b][cap:] == FILL).all(), f"{what}: block {b} wrote past its output region"
        n = min(nsym[b], cap)
        assert dout[b][:n].tobytes() == hout[b][:n].tobytes(), f"{what}: block {b} bytes differ"


def encode_blocks(shafa, oracle, blocks, tables):
    """Streams of `blocks` under `tables` (oracle encoder) -> list of uint8 arrays."""
    out = []
    for data, t in zip(blocks, tables):
        rc, s = oracle.sf_encode(data, t) if data.size else (0, np.zeros(0, dtype=np.uint8))
        assert rc == 0
        out.append(np.ascontiguousarray(s, dtype=np.uint8))
    return out


def run_cases(shafa, streams, tables, nsym, in_cap=None, out_cap=None, dev_in_n=None, dev_nsym=None, what=""):
    import torch
    st = torch.cuda.Stream(device=_dev())
    in_n = [s.size for s in streams]
    in_cap = in_cap or in_n
    out_cap = out_cap or [max(n, 1) for n in nsym]
    off, d_in = _upload(streams, in_cap)
    bt = shafa.Batch(len(streams), max(max(in_cap), max(out_cap), 1))
    host, dev = decode_both(shafa, bt, st, d_in, off, in_cap, dev_in_n or in_n, tables, dev_nsym or nsym, out_cap)
    bt.close()
    check_same(host, dev, dev_nsym or nsym, out_cap, what)
    return host, dev


# ---- F -> T -> C -> D on the device, one synchronisation -------------------------------------------------------------
def chain(shafa, oracle, blocks, rle):
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
        d_cn = _i64(sizes)
    toff, tpos = layout([shafa.tile_hist_bytes(c) for c in ccap])
    d_th = torch.zeros(tpos + 16, dtype=torch.uint8, device=dev)
    ecap = [c * 3 + 16 for c in ccap]
    eoff, epos = layout(ecap)
    d_e = torch.zeros(epos, dtype=torch.uint8, device=dev)
    d_en = torch.zeros(nb, dtype=torch.int64, device=dev)
    doff, dpos = layout(ccap, pad=GUARD)
    d_d = torch.full((dpos + GUARD,), FILL, dtype=torch.uint8, device=dev)
    ooff, opos = layout(sizes, pad=GUARD)
    d_o = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=dev)
    d_on = torch.zeros(nb, dtype=torch.int64, device=dev)
    bt = shafa.Batch(nb, max(max(ecap), 1))
    if rle:
        bt.rle_encode_tiles(st, d_in, off, sizes, d_c, coff, ccap, d_cn, d_freq, d_th, toff)
    else:
        bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
    bt.sf_build_codes(st, nb, d_freq, d_tab)
    bt.sf_encode_dev(st, d_c, coff, ccap, d_cn, d_tab, d_e, eoff, ecap, d_en, d_th, toff)
    bt.sf_decode_dev(st, d_e, eoff, ecap, d_en, d_tab, d_cn, d_d if rle else d_o, doff if rle else ooff,
                     ccap if rle else sizes)
    if rle:
        bt.rle_decode_dev(st, d_d, doff, ccap, d_cn, d_o, ooff, sizes, d_on)
    _, errs = bt.finish(st, nb, raise_on_error=False)
    bt.close()
    out = d_o.cpu().numpy()
    on = d_on.cpu().numpy()
    cn = d_cn.cpu().numpy()
    tabs = d_tab.cpu().numpy().reshape(nb, tsz)
    for i, b in enumerate(blocks):
        if cn[i] > 0 and tabs[i, :256].max() == 0:       # one distinct symbol: no code, the reference's decoder refuses it
            assert errs[i] == shafa.FILE_UNRECOGNIZABLE, (i, errs)
            continue
        assert errs[i] == 0, (i, errs)
        got = out[ooff[i]:ooff[i] + sizes[i]]
        assert got.tobytes() == b.tobytes(), f"block {i} ({sizes[i]} B) round trip differs"
        assert (out[ooff[i] + sizes[i]:ooff[i] + (sizes[i] + 15) // 16 * 16 + GUARD] == FILL).all()
        if rle:
            assert int(on[i]) == sizes[i]


SMALL_SIZES = [0, 1, 15, 8191, 8192, 8193, 100000 + 7, 3 * 32768 + 4095]


@pytest.mark.parametrize("rle", [False, True])
def test_chain_small_blocks(oracle, shafa, rle):
    synth = __import__("pkgload").load_submodule("synth")
    gens = dict(_streams(oracle, shafa))
    gens["mixed"] = lambda n, s: synth.mixed_file_stream(s, n)
    blocks = []
    for k, (name, g) in enumerate(gens.items()):
        for j, n in enumerate(SMALL_SIZES):
            blocks.append(np.ascontiguousarray(g(n, 2000 + 17 * k + j), dtype=np.uint8))
    chain(shafa, oracle, blocks, rle)


def test_chain_large_blocks(oracle, shafa):
    zt = shafa.zipf_table(1.2)
    sizes = [8 << 20, (8 << 20) - 5, 64 << 20]
    chain(shafa, oracle, [oracle.gen_bytes(300 + i, n, zt) for i, n in enumerate(sizes)], False)


def test_chain_128_blocks(oracle, shafa):
    zt = shafa.zipf_table(1.2)
    chain(shafa, oracle, [oracle.gen_bytes(500 + i, 20000 + 3331 * (i % 7), zt) for i in range(128)], False)


# ---- hand-made tables of every class in one launch -------------------------------------------------------------------
def handmade(oracle, shafa):
    blocks, tabs = [], []
    u = oracle.gen_bytes(7, 70000)
    blocks.append(u)
    tabs.append(oracle.sf_build(oracle.hist256(u)))                                       # 9 bits (uniform)
    for nsyms, n, seed in ((9, 30000, 6), (11, 50000, 1), (13, 40000, 8), (14, 90001, 2), (16, 33000, 3),
                           (17, 65536 + 9, 7), (24, 120000, 4), (60, 70001, 5)):
        ot, data = long_code_case(oracle, n, nsyms, 0.5, seed)
        blocks.append(data)
        tabs.append(ot)
    zt = shafa.zipf_table(1.2)
    z = oracle.gen_bytes(11, 40000, zt)
    blocks.append(z)
    tabs.append(oracle.sf_build(oracle.hist256(z)))
    streams = encode_blocks(shafa, oracle, blocks, tabs)
    tables = [to_shafa_table(shafa, t) for t in tabs]
    nsym = [b.size for b in blocks]
    lm = [max(bytes(t.len)) for t in tables]
    assert any(x > 32 for x in lm) and any(17 <= x <= 32 for x in lm) and any(13 <= x <= 16 for x in lm), lm
    return streams, tables, nsym


def _copy(shafa, t):
    return shafa.CodeTable.from_buffer_copy(bytes(t))


def test_handmade_tables_every_class(oracle, shafa):
    streams, tables, nsym = handmade(oracle, shafa)
    z_stream, zt = streams[-1], tables[-1]
    used = [s for s in range(256) if zt.len[s]]
    a, b2 = used[0], used[1]
    dup = _copy(shafa, zt)                                              # duplicate code
    dup.len[b2] = dup.len[a]
    for q in range(32):
        dup.bits[b2][q] = dup.bits[a][q]
    pre = _copy(shafa, zt)                                              # a code that is a prefix of another
    pre.len[a] = max(1, zt.len[a] - 1)
    leaf = _copy(shafa, zt)                                             # a path through a leaf
    leaf.len[b2] = zt.len[a] + 2
    for q in range(32):
        leaf.bits[b2][q] = zt.bits[a][q]
    incomplete = _copy(shafa, zt)                                       # a missing symbol: incomplete code
    incomplete.len[used[-1]] = 0
    single = shafa.CodeTable()
    single.len[65] = 1                                                  # one symbol, code '0'
    extra = [
        (z_stream, dup, nsym[-1]), (z_stream, pre, nsym[-1]), (z_stream, leaf, nsym[-1]), (z_stream, incomplete, nsym[-1]),
        (z_stream, shafa.CodeTable(), 100),                                           # empty table with symbols
        (np.zeros(64, dtype=np.uint8), single, 500),                                  # single symbol
        (np.zeros(0, dtype=np.uint8), zt, 100),                                       # empty stream with symbols
        (z_stream, dup, 0),                                                           # malformed, nothing to decode
    ]
    streams = streams + [e[0] for e in extra]
    tables = tables + [e[1] for e in extra]
    nsym = nsym + [e[2] for e in extra]
    for speculate in (1, 2, 0):
        shafa.set_option("sf_decode_speculate", speculate)
        try:
            host, dev = run_cases(shafa, streams, tables, nsym, what=f"speculate={speculate}")
        finally:
            shafa.set_option("sf_decode_speculate", 1)
        assert dev[0][:10] == [0] * 10
        assert dev[0][10] == shafa.FILE_UNRECOGNIZABLE and dev[0][14] == shafa.FILE_UNRECOGNIZABLE, dev[0]


def test_several_bytemap_blocks_and_memory_rule(oracle, shafa):
    """Incomplete and 17..32-bit blocks share the byte-map list; of the > 32-bit blocks only the first with symbols runs."""
    blocks, tabs = [], []
    for nsyms, n, seed in ((24, 120000, 4), (20, 30001, 9), (60, 70001, 5), (50, 5000, 3), (45, 262144 + 3, 2)):
        ot, data = long_code_case(oracle, n, nsyms, 0.5, seed)
        blocks.append(data)
        tabs.append(ot)
    streams = encode_blocks(shafa, oracle, blocks, tabs)
    tables = [to_shafa_table(shafa, t) for t in tabs]
    nsym = [b.size for b in blocks]
    inc = _copy(shafa, tables[1])
    inc.len[[s for s in range(256) if inc.len[s]][-1]] = 0
    streams.append(streams[1])
    tables.append(inc)
    nsym.append(nsym[1])
    import torch
    st = torch.cuda.Stream(device=_dev())
    in_n = [s.size for s in streams]
    off, d_in = _upload(streams, in_n)
    bt = shafa.Batch(len(streams), max(max(in_n), max(nsym)))
    ooff, opos = layout(nsym, pad=GUARD)
    d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
    bt.sf_decode_dev(st, d_in, off, in_n, _i64(in_n), _tables_dev(tables), _i64(nsym), d_out, ooff, nsym)
    _, errs = bt.finish(st, len(streams), raise_on_error=False)
    out = d_out.cpu().numpy()
    assert errs == [0, 0, 0, shafa.LACK_OF_MEMORY, shafa.LACK_OF_MEMORY, errs[5]], errs   # 59 / 49 / 44 bits: one slot
    for i in (0, 1, 2):
        assert out[ooff[i]:ooff[i] + nsym[i]].tobytes() == blocks[i].tobytes(), f"block {i}"
    for i in (3, 4):
        assert (out[ooff[i]:ooff[i] + nsym[i] + GUARD] == FILL).all(), f"block {i} was written"
    # each lone > 32-bit block decodes at its full size
    for i in (3, 4):
        host, dev = run_cases(shafa, [streams[i]], [tables[i]], [nsym[i]], what=f"lone block {i}")
        assert dev[0] == [0] and dev[1][0][:nsym[i]].tobytes() == blocks[i].tobytes()
    # the incomplete block against the host entry
    run_cases(shafa, streams[:3] + streams[5:], tables[:3] + tables[5:], nsym[:3] + nsym[5:], what="bytemap mix")
    bt.close()


# ---- damaged streams, capacities, knobs ------------------------------------------------------------------------------
def test_damaged_streams(oracle, shafa):
    zt = shafa.zipf_table(1.2)
    rng = np.random.default_rng(77)
    blocks = [oracle.gen_bytes(60 + i, n, zt) for i, n in enumerate((50000, 200000, 9000))]
    u = oracle.gen_bytes(66, 40000)
    blocks.append(u)
    tabs = [oracle.sf_build(oracle.hist256(b)) for b in blocks]
    streams = encode_blocks(shafa, oracle, blocks, tabs)
    tables = [to_shafa_table(shafa, t) for t in tabs]
    s_trunc, s_flip, s_more = [], [], []
    for s, b in zip(streams, blocks):
        f = s.copy()
        idx = rng.integers(0, s.size, 20)
        f[idx] ^= (1 << rng.integers(0, 8, 20)).astype(np.uint8)
        s_flip.append(f)
    n = [b.size for b in blocks]
    cut = [max(1, s.size * 3 // 5) for s in streams]
    cases = streams + s_flip + streams + streams
    in_n = [s.size for s in streams] + [s.size for s in streams] + cut + [s.size for s in streams]
    nsym = n + n + n + [x + 5000 for x in n]
    for speculate in (1, 2, 0):
        shafa.set_option("sf_decode_speculate", speculate)
        try:
            run_cases(shafa, cases, tables * 4, nsym, in_cap=[s.size for s in cases], out_cap=nsym,
                      dev_in_n=in_n, what=f"damaged speculate={speculate}")
        finally:
            shafa.set_option("sf_decode_speculate", 1)


def test_past_capacity(oracle, shafa):
    import torch
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(80 + i, 30000, zt) for i in range(3)]
    tabs = [oracle.sf_build(oracle.hist256(b)) for b in blocks]
    streams = encode_blocks(shafa, oracle, blocks, tabs)
    tables = [to_shafa_table(shafa, t) for t in tabs]
    in_cap = [s.size for s in streams]
    in_n = [in_cap[0] + 1, in_cap[1], in_cap[2]]
    nsym = [30000, 30001, 30000]
    out_cap = [30000, 30000, 30000]
    st = torch.cuda.Stream(device=_dev())
    off, d_in = _upload(streams, in_cap)
    ooff, opos = layout(out_cap, pad=GUARD)
    d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
    bt = shafa.Batch(3, 1 << 20)
    bt.sf_decode_dev(st, d_in, off, in_cap, _i64(in_n), _tables_dev(tables), _i64(nsym), d_out, ooff, out_cap)
    _, errs = bt.finish(st, 3, raise_on_error=False)
    bt.close()
    out = d_out.cpu().numpy()
    assert errs == [shafa.OUTSIDE_MODULE, shafa.OUTSIDE_MODULE, 0], errs
    for i in (0, 1):
        assert (out[ooff[i]:ooff[i] + 30000 + GUARD] == FILL).all()
    assert out[ooff[2]:ooff[2] + 30000].tobytes() == blocks[2].tobytes()


@pytest.mark.parametrize("knob,value", [("sf_decode_path", 1), ("sf_decode_path", 2), ("sf_decode_speculate", 0),
                                        ("sf_decode_speculate", 2)])
def test_knobs(oracle, shafa, knob, value):
    streams, tables, nsym = handmade(oracle, shafa)
    shafa.set_option(knob, value)
    try:
        host, dev = run_cases(shafa, streams, tables, nsym, what=f"{knob}={value}")
    finally:
        shafa.set_option(knob, 0 if knob == "sf_decode_path" else 1)
    assert dev[0] == [0] * len(streams)


# ---- rle_decode_dev ---------------------------------------------------------------------------------------------------
def test_rle_decode_dev_against_rle_decode(oracle, shafa):
    import torch
    synth = __import__("pkgload").load_submodule("synth")
    zt = shafa.zipf_table(1.2)
    raw = [synth.runs_stream(90 + i, n, zt) for i, n in enumerate((100000, 70000, 5000, 300000))]
    encs = []
    for r in raw:
        encs.append(np.ascontiguousarray(oracle.rle_encode(r), dtype=np.uint8))
    cut = encs[0][:-1].copy()                                           # a cut triple (if it ends in one) / shorter stream
    cases = encs + [cut, np.zeros(0, dtype=np.uint8), encs[1], encs[3]]
    out_cap = [r.size for r in raw] + [raw[0].size, 16, raw[1].size // 2, (64 << 20) + 4096]
    in_n = [c.size for c in cases]
    in_cap = in_n[:]
    dev_n = in_n[:]
    cases.append(encs[2])                                               # past capacity
    in_cap.append(encs[2].size)
    in_n.append(encs[2].size)
    dev_n.append(encs[2].size + 1)
    out_cap.append(raw[2].size)
    st = torch.cuda.Stream(device=_dev())
    off, d_in = _upload(cases, in_cap)
    ooff, opos = layout(out_cap, pad=GUARD)
    nb = len(cases)
    bt = shafa.Batch(nb, max(out_cap))
    res = []
    for which in ("host", "dev"):
        d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
        d_on = torch.full((nb,), -1, dtype=torch.int64, device=_dev())
        if which == "host":
            bt.rle_decode(st, d_in, off, in_n[:-1] + [0], d_out, ooff, out_cap, d_on)
        else:
            bt.rle_decode_dev(st, d_in, off, in_cap, _i64(dev_n), d_out, ooff, out_cap, d_on)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        res.append((errs, d_on.cpu().numpy(), d_out.cpu().numpy()))
    bt.close()
    (herr, hn, hout), (derr, dn, dout) = res
    assert derr[:-1] == herr[:-1], (herr, derr)
    assert derr[-1] == shafa.OUTSIDE_MODULE and dn[-1] == 0
    assert (dout[ooff[-1]:ooff[-1] + out_cap[-1] + GUARD] == FILL).all()
    for i in range(nb - 1):
        assert dn[i] == hn[i], (i, dn[i], hn[i])
        n = min(int(hn[i]), out_cap[i])
        assert dout[ooff[i]:ooff[i] + n].tobytes() == hout[ooff[i]:ooff[i] + n].tobytes(), f"block {i}"
        assert (dout[ooff[i] + out_cap[i]:ooff[i] + (out_cap[i] + 15) // 16 * 16 + GUARD] == FILL).all()
    for i in range(4):
        assert derr[i] == 0 and dout[ooff[i]:ooff[i] + raw[i].size].tobytes() == raw[i].tobytes()


# ---- files the reference wrote -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,stem,rle", [("runs_default", "x", True), ("uniform_no_rle", "u", False),
                                           ("textlike_m", "t", False)])
def test_reference_files(shafa, case, stem, rle):
    import torch
    data = rd(case, stem)
    fstem = stem + (".rle" if rle else "")
    _, cblocks = parse_blocks_text(rd(case, fstem + ".cod"))
    payloads = parse_shaf(rd(case, fstem + ".shaf"))
    tables, sizes = [], []
    for size, ctext in cblocks:
        rc, tab = shafa.cod_parse(ctext)
        assert rc == 0
        tables.append(tab)
        sizes.append(size)
    nb = len(payloads)
    streams = [np.frombuffer(p, dtype=np.uint8) for p in payloads]
    in_n = [s.size for s in streams]
    off, d_in = _upload(streams, in_n)
    st = torch.cuda.Stream(device=_dev())
    doff, dpos = layout(sizes)
    d_d = torch.zeros(dpos + 16, dtype=torch.uint8, device=_dev())
    d_sizes = _i64(sizes)
    bt = shafa.Batch(nb, max(max(sizes), (64 << 20) + 1024) if rle else max(sizes))
    bt.sf_decode_dev(st, d_in, off, in_n, _i64(in_n), _tables_dev(tables), d_sizes, d_d, doff, sizes)
    if rle:
        ocap = [(64 << 20) + 1024] * nb
        ooff, opos = layout(ocap)
        d_o = torch.zeros(opos, dtype=torch.uint8, device=_dev())
        d_on = torch.zeros(nb, dtype=torch.int64, device=_dev())
        bt.rle_decode_dev(st, d_d, doff, sizes, d_sizes, d_o, ooff, ocap, d_on)
    bt.finish(st, nb)
    bt.close()
    if rle:
        out, on = d_o.cpu().numpy(), d_on.cpu().numpy()
        got = b"".join(out[o:o + int(n)].tobytes() for o, n in zip(ooff, on))
    else:
        out = d_d.cpu().numpy()
        got = b"".join(out[o:o + n].tobytes() for o, n in zip(doff, sizes))
    assert got == data


# ---- enqueue only ------------------------------------------------------------------------------------------------------
def test_no_synchronisation_inside_the_calls(oracle, shafa):
    """F -> T -> C -> D enqueues and returns while the stream is still busy; one synchronisation at the end."""
    import torch
    dev = _dev()
    zt = shafa.zipf_table(1.2)
    blocks = [oracle.gen_bytes(900 + i, 1 << 20, zt) for i in range(4)]
    sizes = [b.size for b in blocks]
    nb = len(blocks)
    off, d_in = _upload(blocks, sizes)
    d_n_in = _i64(sizes)
    tsz = C.sizeof(shafa.CodeTable)
    d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
    d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    toff, tpos = layout([shafa.tile_hist_bytes(n) for n in sizes])
    d_th = torch.zeros(tpos, dtype=torch.uint8, device=dev)
    caps = [n * 2 + 16 for n in sizes]
    eoff, epos = layout(caps)
    d_e = torch.zeros(epos, dtype=torch.uint8, device=dev)
    d_en = torch.zeros(nb, dtype=torch.int64, device=dev)
    ooff, opos = layout(sizes)
    d_o = torch.zeros(opos, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(nb, max(caps))

    def enqueue():
        bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
        bt.sf_build_codes(st, nb, d_freq, d_tab)
        bt.sf_encode_dev(st, d_in, off, sizes, d_n_in, d_tab, d_e, eoff, caps, d_en, d_th, toff)
        bt.sf_decode_dev(st, d_e, eoff, caps, d_en, d_tab, d_n_in, d_o, ooff, sizes)

    enqueue()                                                                             # warm-up: the batch grows here
    bt.finish(st, nb)
    d_o.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)
    enqueue()
    busy = not st.query()
    bt.finish(st, nb)
    assert busy, "the stream had drained when the calls returned: something synchronised"
    out = d_o.cpu().numpy()
    for i, b in enumerate(blocks):
        assert out[ooff[i]:ooff[i] + sizes[i]].tobytes() == b.tobytes()
    bt.close()


def _unary_case(shafa, nsyms, n, seed):
    """A hand-made table whose symbol i has the code 1^i 0 (length i + 1; the last symbol 1^(nsyms-1)), and a stream of n
    symbols coded with it, bit-packed MSB first."""
    t = shafa.CodeTable()
    for i in range(nsyms):
        L = i + 1 if i < nsyms - 1 else nsyms - 1
        t.len[i] = L
        for q in range(min(i, L)):
            t.bits[i][q >> 3] |= 0x80 >> (q & 7)
    rng = np.random.default_rng(seed)
    data = np.minimum(rng.geometric(0.5, n) - 1, nsyms - 1).astype(np.uint8)
    data[:nsyms] = np.arange(nsyms, dtype=np.uint8)
    bits = []
    for s in data:
        L = int(t.len[s])
        bits.extend(1 if q < min(int(s), L) else 0 for q in range(L))
    return t, data, np.packbits(np.array(bits, dtype=np.uint8))


def test_memory_rule_at_its_boundary(shafa):
    """Codes of 33..64 bits: the slot goes to the first block that would decode, so an earlier such block past its
    capacity does not take it; codes of more than 64 bits are SHAFA_LACK_OF_MEMORY with nothing written."""
    import torch
    t64, d64, s64 = _unary_case(shafa, 64, 20000, 1)
    t40, d40, s40 = _unary_case(shafa, 40, 30000, 2)
    t70, d70, s70 = _unary_case(shafa, 70, 5000, 3)
    assert max(bytes(t64.len)) == 63 and max(bytes(t70.len)) == 69
    streams = [s40, s64, s70]
    tables = [t40, t64, t70]
    nsym = [d40.size, d64.size, d70.size]
    in_cap = [s.size for s in streams]
    dev_in_n = [in_cap[0] + 1, in_cap[1], in_cap[2]]                  # block 0: past its capacity, never decoded
    st = torch.cuda.Stream(device=_dev())
    off, d_in = _upload(streams, in_cap)
    ooff, opos = layout(nsym, pad=GUARD)
    d_out = torch.full((opos + GUARD,), FILL, dtype=torch.uint8, device=_dev())
    bt = shafa.Batch(3, max(max(in_cap), max(nsym)))
    bt.sf_decode_dev(st, d_in, off, in_cap, _i64(dev_in_n), _tables_dev(tables), _i64(nsym), d_out, ooff, nsym)
    _, errs = bt.finish(st, 3, raise_on_error=False)
    out = d_out.cpu().numpy()
    assert errs == [shafa.OUTSIDE_MODULE, 0, shafa.LACK_OF_MEMORY], errs
    assert out[ooff[1]:ooff[1] + nsym[1]].tobytes() == d64.tobytes()
    for i in (0, 2):
        assert (out[ooff[i]:ooff[i] + nsym[i] + GUARD] == FILL).all(), f"block {i} was written"
    # the host entry decodes the 69-bit block; a lone 63-bit block at its capacity decodes on the device too
    host, _ = decode_both(shafa, bt, st, d_in, off, in_cap, in_cap, tables, nsym, nsym)
    bt.close()
    assert host[0][2] == 0 and host[1][2][:nsym[2]].tobytes() == d70.tobytes()
    run_cases(shafa, [s64], [t64], [nsym[1]], what="lone 63-bit block")
