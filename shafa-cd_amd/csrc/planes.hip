// planes.hip — arrays of E-byte elements <-> their E byte planes (shafa_hipd_split_planes_dev, shafa_hipd_merge_planes_dev), and
// the same with every element XORed with the element of a base region (the _xor_dev entries: tensor deltas).
//
// Block b is d_n[b] (<= cap[b]) elements of E = 1, 2, 4 or 8 bytes.  ELEMENT SIDE: its E d_n[b] bytes at d_el + off[b], at ANY
// byte alignment, never copied: split reads the aligned 16-byte words around what a lane wants and shifts them into place
// (shift_words, as find.hip and crc32.hip do); merge stores aligned 16-byte words that lie wholly inside the region and single
// bytes at its two ends.  PLANE SIDE: plane j (byte j of every element, plane 0 the least significant) is d_n[b] bytes at
// d_planes + poff[b E + j], every one a multiple of 16, so a lane's 16 bytes of a plane are one aligned word.
//
// The unit is 16 elements a lane: E words of the element side, v_perm_b32 in registers, one word of each plane — per plane a
// wave's 64 words are 1 KiB contiguous.  A tile is tile_pass.hpp's 256 lanes x 32, here ELEMENTS: two units a lane, 4096
// elements apart, so that both passes over a plane stay contiguous across the workgroup.  The tiles of all blocks are numbered
// from the capacities on the host (TpWalk) and dealt to the workgroups in equal runs; an empty or short tile exits.  One
// launch, no workgroup waits for another; the only atomic is the error word of a block with d_n[b] > cap[b], of which no byte
// is read or written.
//
// What the measurements settled.  split's element-side loads: a lane's E words are 16 E bytes apart from its
// neighbour's, so one load instruction touches every E-th word of the lines it reads; a whole pass of a 16-aligned region goes
// through LDS instead (split_pass_lds: coalesced loads, 4.8 -> 5.4 TB/s at 2 bytes, 3.6 -> 5.1 TB/s at 4), every other unit —
// an unaligned region, the pass a block ends in — loads directly.  Stores: the planes' are whole lines and streamed
// (non-temporal: + 5 .. 8 %); merge's element-side stores are the strided ones, and non-temporal they leave L2 a word at a
// time (1.3 TB/s at 4 bytes against 4.3 TB/s plain, where L2 puts the lines together): plain.
//
// merge: a lane's 16 E bytes start at byte 16 g E of the region (g the unit's number in the block), i.e. sh = (address of the
// region) mod 16 bytes behind an aligned word.  The lane owns the E aligned words that START in its unit's span shifted down by
// sh: their first sh bytes are the last bytes of unit g - 1 — the lane in front's, by four shuffles; a wave's first lane loads
// and merges that unit's tail itself — and the unit's own last sh bytes are left to the lane behind, or, in the block's last
// unit, stored as bytes.  A word that reaches in front of the region or past the unit's last element is stored as bytes too.
// Algorithmic HBM bytes: every element read once and written once.
//
// With a base (template XOR): block b's base region is its own E d_n[b] bytes at d_base + boff[b], at an alignment of
// ITS own, read once the way split reads the element side (xor_base); a block whose boff is SHAFA_PLANES_NO_BASE has none and
// goes through as in the plain kernels.  split XORs the base onto the elements right after they are shifted into place — in a
// pass where both regions are 16-aligned the base takes the coalesced path through LDS behind the element side — and merge onto
// the rebuilt elements in front of the shift to the output's alignment.  3 bytes of traffic per tensor byte.  The plain entries
// launch the XOR = false instantiations, from which every trace of the base is compiled out.
//
// Differences (template DIFF, the _diff_dev entries): the planes are those of z[i], the zigzag fold of
// d[i] = x[i] - x[i-1] mod M, x the block's elements as unsigned little-endian integers, M = 2^(8 E), x[-1] = 0.  split subtracts
// and folds on its element-ordered dwords in front of split_store; the element in front of a lane's unit is the last one of the
// LDS word in front in the coalesced pass (the pass's first lane loads it), and elsewhere the lane in front's last one, by shuffle
// (a wave's first lane loads it itself) — one launch, 2 bytes of traffic per tensor byte.
// merge needs every element's prefix sum and no workgroup may wait for another, so it is three launches: the sum of the d's of
// every tile (planes_diff_sums), each block's sums turned into exclusive prefixes (planes_diff_scan, one workgroup a block),
// and the plain merge's structure with a scan over the tile in element order on top of the tile's prefix (planes_merge_diff) —
// the planes are read twice, 3 bytes of traffic per tensor byte.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"
#include "planes_arith.hpp"

namespace {

// w ^= bytes p .. p + 16 W - 1 of the base region of nbytes bytes at bs, which lies at an alignment of its own: read as split
// reads its element side, the quarter of the shift (uniform) picked around the shifts alone.  The loads are plain: a lane's words
// are 16 W bytes from its neighbour's, the rest of a line comes with the instructions that follow, and streamed loads let the
// line go in between (8 to 22 % slower).  Base bytes behind the region end up in dwords of w behind the block's
// last element, which no caller stores.
template <int W>
__device__ __forceinline__ void xor_base(const u8 *bs, u64 nbytes, u64 p, u32 *w)
{
    const u32 sh = (u32)((uintptr_t)bs & 15u), r = sh & 3u;
    uint4 a[W + 1];
    load_words<W, false>(bs, nbytes, p, sh, a);
    switch (sh >> 2) {                               // uniform
    case 0: shift_into<W, 0, true>(a, r, w); break;
    case 1: shift_into<W, 1, true>(a, r, w); break;
    case 2: shift_into<W, 2, true>(a, r, w); break;
    default: shift_into<W, 3, true>(a, r, w); break;
    }
}

// The unit of 16 elements from element e0 < n of a region of n elements at src (src mod 16 = 4 Q + r) -> its E plane words.
// An aligned word of the element side is read only where it holds a byte of the region; what such a word holds behind the
// region ends up in plane bytes behind n, which are not stored.  bs (XOR: the block's base region, or NULL): the elements are
// XORed with the base's in element order as soon as they are in place, so only one side's E + 1 words are live at a time.
// DIFF: the planes of the folded differences; the callers' active lanes are a wave's first ones, so the lane in front holds a unit.
template <int E, int Q, bool XOR, bool DIFF>
__device__ __forceinline__ void split_unit(const u8 *src, u64 n, u64 e0, u32 r, const u8 *bs, u8 *d_planes, const u64 *poff)
{
    const u64 nbytes = n * E, p = e0 * E;
    typename DiffT<E>::T own0 = 0;                   // asked for first: it is there when the unit's words are
    if (DIFF && lane_id() == 0 && e0 != 0) own0 = elem_in_front<E>(src, e0);
    u32 w[4 * E];
    {
        uint4 a[E + 1];
        load_words<E, true>(src, nbytes, p, 4u * Q + r, a);
        shift_into<E, Q, false>(a, r, w);
    }
    if (XOR && bs) xor_base<E>(bs, nbytes, p, w);    // (uniform)
    if (DIFF) diff_fold<E>(w, prev_of<E>(w, own0));
    split_store<E>(w, n, e0, d_planes, poff);
}

// A whole pass (every lane a whole unit) of a 16-aligned region: the pass's 4096 E bytes are loaded as E coalesced words a
// lane (a wave reads 1 KiB contiguous) and handed over through LDS, where lane l reads its own words l E .. l E + E - 1.  One
// slot of padding every 16 keeps both sides free of bank conflicts: a 16-lane group of the strided reads covers 16 rows or all
// 16 slots of E rows.  bs (XOR: the base region, 16-aligned too, or NULL): the base's pass follows through the same rows in a
// second round and is XORed onto the lane's words.  (XORing the two coalesced words in front of one round through LDS is
// less LDS traffic and two barriers fewer, but keeps 2 E loads in flight a lane: 6 % slower at 4 bytes, no faster at 2.)
constexpr int PL_LDS_SLOTS = TP_THREADS + TP_THREADS / 16;      // per byte of the element
template <int E, bool XOR, bool DIFF>
__device__ __forceinline__ void split_pass_lds(const u8 *src, u64 n, u64 e0_pass, const u8 *bs, u8 *d_planes, const u64 *poff,
                                               uint4 *lds)
{
    const u32 tid = threadIdx.x;
    const u8 *base = src + e0_pass * E;
    // DIFF: the element in front of a lane's unit is the last one of the LDS word in front of its own; the pass's first lane
    // loads it (one load: the region is 16-aligned), asked for first so that it is there when the pass's words are
    typename DiffT<E>::T prev = 0;
    if (DIFF && tid == 0 && e0_pass != 0) {
        if (E == 8) prev = (typename DiffT<E>::T)gload<u64>(base - 8);
        else if (E == 4) prev = gload<u32>(base - 4);
        else if (E == 2) prev = gload<u16>(base - 2);
        else prev = gload<u8>(base - 1);
    }
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const u32 wd = (u32)i * TP_THREADS + tid;
        lds[wd + (wd >> 4)] = gload_nt<uint4>(base + 16ull * wd);
    }
    lds_barrier();
    u32 w[4 * E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const u32 wd = tid * E + (u32)i;
        const uint4 v = lds[wd + (wd >> 4)];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    if (DIFF && tid != 0) {
        const u32 wd = tid * E - 1;
        const u32 *last = (const u32 *)&lds[wd + (wd >> 4)];
        if (E == 8) prev = (typename DiffT<E>::T)((u64)last[3] << 32 | last[2]);
        else prev = last[3] >> (32 - 8 * E);
    }
    lds_barrier();
    if (XOR && bs) {                                 // (uniform)
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const u32 wd = (u32)i * TP_THREADS + tid;
            lds[wd + (wd >> 4)] = gload_nt<uint4>(bs + e0_pass * E + 16ull * wd);
        }
        lds_barrier();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const u32 wd = tid * E + (u32)i;
            const uint4 v = lds[wd + (wd >> 4)];
            w[4 * i] ^= v.x; w[4 * i + 1] ^= v.y; w[4 * i + 2] ^= v.z; w[4 * i + 3] ^= v.w;
        }
        lds_barrier();
    }
    if (DIFF) diff_fold<E>(w, prev);
    split_store<E>(w, n, e0_pass + (u64)tid * PL_UNIT, d_planes, poff);
}

template <int E, int Q, bool XOR, bool DIFF>
__device__ __forceinline__ void split_tile(const TpWalk &wk, u32 r, const u8 *bs, u8 *d_planes, const u64 *poff, uint4 *lds)
{
    const bool both16 = Q == 0 && r == 0 && (!XOR || ((uintptr_t)bs & 15u) == 0);     // a block without a base: bs is NULL
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        if (both16 && wk.pos0 + (u64)(u + 1) * PL_PASS <= wk.n) {                    // (uniform) the barriers are inside
            split_pass_lds<E, XOR, DIFF>(wk.in, wk.n, wk.pos0 + (u64)u * PL_PASS, bs, d_planes, poff, lds);
            continue;
        }
        const u64 e0 = wk.pos0 + (u64)u * PL_PASS + (u64)threadIdx.x * PL_UNIT;
        if (e0 < wk.n) split_unit<E, Q, XOR, DIFF>(wk.in, wk.n, e0, r, bs, d_planes, poff);
    }
}

// block b's base region (the XOR launches): NULL where its offset says that it has none, and then d_base is not looked at
__device__ __forceinline__ const u8 *base_of(const u8 *d_base, const u64 *d_boff, int b)
{
    const u64 o = d_boff[b];
    return o == SHAFA_PLANES_NO_BASE ? nullptr : d_base + o;
}

// the split kernels' body.  XOR: block b's base region at d_base + d_boff[b]; DIFF: the folded differences
template <int E, bool XOR, bool DIFF>
__device__ __forceinline__ void split_blocks(const u8 *__restrict__ d_el, const u64 *__restrict__ off, const u64 *__restrict__ cap,
                                             const u32 *__restrict__ tbase, int nblk, const u64 *__restrict__ d_n,
                                             u8 *__restrict__ d_planes, const u64 *__restrict__ d_poff, int *__restrict__ err,
                                             u32 n_tiles, u32 per_wg, const u8 *__restrict__ d_base,
                                             const u64 *__restrict__ d_boff, uint4 *lds)
{
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        const u8 *bs = XOR ? base_of(d_base, d_boff, wk.b) : nullptr;
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: split_tile<E, 0, XOR, DIFF>(wk, r, bs, d_planes, poff, lds); break;
        case 1: split_tile<E, 1, XOR, DIFF>(wk, r, bs, d_planes, poff, lds); break;
        case 2: split_tile<E, 2, XOR, DIFF>(wk, r, bs, d_planes, poff, lds); break;
        default: split_tile<E, 3, XOR, DIFF>(wk, r, bs, d_planes, poff, lds); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// XOR: the _xor entry's launch; the plain entry's passes neither d_base nor d_boff
template <int E, bool XOR>
__global__ __launch_bounds__(TP_THREADS) void planes_split(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                           const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                           const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                           const u64 *__restrict__ d_poff, int *__restrict__ err, u32 n_tiles,
                                                           u32 per_wg, const u8 *__restrict__ d_base,
                                                           const u64 *__restrict__ d_boff)
{
    __shared__ uint4 lds[PL_LDS_SLOTS * E];
    split_blocks<E, XOR, false>(d_el, off, cap, tbase, nblk, d_n, d_planes, d_poff, err, n_tiles, per_wg, d_base, d_boff, lds);
}

// the _diff entry's launch
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_split_diff(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                int nblk, const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                                const u64 *__restrict__ d_poff, int *__restrict__ err, u32 n_tiles,
                                                                u32 per_wg)
{
    __shared__ uint4 lds[PL_LDS_SLOTS * E];
    split_blocks<E, false, true>(d_el, off, cap, tbase, nblk, d_n, d_planes, d_poff, err, n_tiles, per_wg, nullptr, nullptr, lds);
}

// bytes 4 Q + r .. + 15 of the dwords at x (Q = 4: r = 0, the word behind)
template <int Q>
__device__ __forceinline__ uint4 shift_at(const u32 *x, u32 r)
{
    return make_uint4(__builtin_amdgcn_alignbyte(x[Q + 1], x[Q], r), __builtin_amdgcn_alignbyte(x[Q + 2], x[Q + 1], r),
                      __builtin_amdgcn_alignbyte(x[Q + 3], x[Q + 2], r), __builtin_amdgcn_alignbyte(x[Q + 4], x[Q + 3], r));
}

// The unit of 16 elements from element e0 of a region of n elements at dst (sh = dst mod 16, 16 - sh = 4 Q + r) <- its E plane
// words.  Every lane of the wave calls (the shuffles); a lane with e0 >= n loads and stores nothing.  bs (XOR: the block's base
// region, or NULL): the unit's bytes are XORed with the base's before they are shifted to dst's alignment, so what a lane hands
// to the lane behind is finished; the tail a wave's first lane rebuilds takes the 16 base bytes in front of the unit.
// DIFF (launch 3 of the merge of differences): the planes are those of the folded differences, and the prefix sums come in
// between.  Then EVERY lane of the workgroup calls (the barrier in wg_excl_scan); a lane with e0 >= n adds 0.  carry: the sum of
// the d's in front of the pass, i.e. the element in front of it.  The scan runs in element order: the lane's 16 elements, the
// lanes of the wave, the waves.  A lane's exclusive prefix IS the element in front of its unit, so a wave's first lane gets the
// last 16 bytes of that unit from it: that unit's last d's, rebuilt from the planes, summed up and taken off.
template <int E, int Q, bool XOR, bool DIFF>
__device__ __forceinline__ void merge_unit(u8 *dst, u64 n, u64 e0, u32 sh, u32 r, const u8 *bs, const u8 *d_planes,
                                           const u64 *poff, typename DiffT<E>::T *carry, typename DiffT<E>::T *wt, u32 *turn)
{
    const bool active = e0 < n;
    // x: [the 16 bytes in front of the unit][the unit's 16 E bytes][zeros]
    u32 x[4 * E + 12];
    u32 p[4 * E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (active) v = gload_nt<uint4>(d_planes + poff[j] + e0);
        p[4 * j] = v.x; p[4 * j + 1] = v.y; p[4 * j + 2] = v.z; p[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int d = 0; d < 4 * E; ++d) x[4 + d] = merge_dword<E>(p, d);
    if (XOR && bs && active) xor_base<E>(bs, n * E, e0 * E, x + 4);
    typename DiffT<E>::T pre = 0;
    if (DIFF) {
        zz_unfold<E, 4 * E>(x + 4);
        const typename DiffT<E>::T tot = scan_incl<E, 4 * E>(x + 4);
        pre = wg_excl_scan<typename DiffT<E>::T>(tot, *carry, wt, *turn);
        add_all<E, 4 * E>(x + 4, pre);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) x[4 * E + 4 + k] = 0;
    if (sh != 0) {                                   // (uniform) the last bytes of the unit in front
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (u32)__shfl_up((int)x[4 * E + k], 1, 64);
        if (lane_id() == 0 && active && e0 != 0) {   // the lane in front is another wave's: that unit is whole
            u32 pp[4 * E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const uint4 v = gload<uint4>(d_planes + poff[j] + e0 - PL_UNIT);
                pp[4 * j] = v.x; pp[4 * j + 1] = v.y; pp[4 * j + 2] = v.z; pp[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = merge_dword<E>(pp, 4 * E - 4 + k);
            if (XOR && bs) xor_base<1>(bs, n * E, e0 * E - 16, x);
            if (DIFF) {
                zz_unfold<E, 4>(x);
                const typename DiffT<E>::T tail = scan_incl<E, 4>(x);          // pre = the element in front of the tail + this
                add_all<E, 4>(x, pre - tail);
            }
        }
    }
    if (!active) return;
    const int cb = (int)(n - e0 >= PL_UNIT ? PL_UNIT : (u32)(n - e0)) * E;      // the unit's bytes
    const bool last = n - e0 <= PL_UNIT;                                       // no lane behind
    const long long ub = (long long)(e0 * E);                                  // the unit's first byte in the region
    // word i holds the region's bytes ub + lo .. + 15, lo = 16 i - sh; word E starts inside the unit only when sh != 0
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        if (i == E && !(last && sh != 0)) break;
        const uint4 o = shift_at<Q>(x + 4 * i, r);
        const int lo = 16 * i - (int)sh;
        if (i < E && ub + lo >= 0 && lo + 16 <= cb) gstore<uint4>(dst + (ub + lo), o);     // plain: see the head of the file
        else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (ub + lo + k >= 0 && lo + k < cb) gstore<u8>(dst + (ub + lo + k), tp_byte_of(o, k));
        }
    }
}

template <int E, int Q, bool XOR>
__device__ __forceinline__ void merge_tile(const TpWalk &wk, u32 sh, u32 r, const u8 *bs, const u8 *d_planes, const u64 *poff)
{
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u64 e0w = wk.pos0 + (u64)u * PL_PASS + (u64)(threadIdx.x & ~63u) * PL_UNIT;
        if (e0w >= wk.n) continue;                   // (wave uniform) no lane of the wave has an element
        merge_unit<E, Q, XOR, false>((u8 *)wk.in, wk.n, e0w + (u64)lane_id() * PL_UNIT, sh, r, bs, d_planes, poff, nullptr,
                                     nullptr, nullptr);
    }
}

template <int E, bool XOR>
__global__ __launch_bounds__(TP_THREADS) void planes_merge(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                           const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                           const u64 *__restrict__ d_n, const u8 *__restrict__ d_planes,
                                                           const u64 *__restrict__ d_poff, int *__restrict__ err, u32 n_tiles,
                                                           u32 per_wg, const u8 *__restrict__ d_base,
                                                           const u64 *__restrict__ d_boff)
{
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        const u8 *bs = XOR ? base_of(d_base, d_boff, wk.b) : nullptr;
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), m = (16u - sh) & 15u, r = m & 3u;
        switch (sh == 0 ? 4u : m >> 2) {             // uniform
        case 0: merge_tile<E, 0, XOR>(wk, sh, r, bs, d_planes, poff); break;
        case 1: merge_tile<E, 1, XOR>(wk, sh, r, bs, d_planes, poff); break;
        case 2: merge_tile<E, 2, XOR>(wk, sh, r, bs, d_planes, poff); break;
        case 3: merge_tile<E, 3, XOR>(wk, sh, r, bs, d_planes, poff); break;
        default: merge_tile<E, 4, XOR>(wk, sh, r, bs, d_planes, poff); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- merge of the differences: three launches, none of which waits for another workgroup
// launch 1: sums[t] = the sum of the d's of global tile t (a tile at or behind its block's size is not read; what the words of
// a block's last unit hold behind its size goes into the block's last sum, which nothing reads)
// SKIP (the grid merge's first pass, planes_lag.hip): a block with d_skip[b] != 0 is the lag family's and left alone
template <int E, bool SKIP = false>
__global__ __launch_bounds__(TP_THREADS) void planes_diff_sums(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                               const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                               const u64 *__restrict__ d_n, const u8 *__restrict__ d_planes,
                                                               const u64 *__restrict__ d_poff, u32 n_tiles, u32 per_wg,
                                                               u64 *__restrict__ sums, const u64 *__restrict__ d_skip)
{
    using T = typename DiffT<E>::T;
    __shared__ T wsum[TP_THREADS / 64];
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (SKIP && d_skip[wk.b]) continue;          // (uniform)
        const u64 *poff = d_poff + (u64)wk.b * E;
        T s = 0;
#pragma unroll
        for (int u = 0; u < PL_UNITS; ++u) {
            const u64 e0 = wk.pos0 + (u64)u * PL_PASS + (u64)threadIdx.x * PL_UNIT;
            if (e0 >= wk.n) continue;
            u32 p[4 * E], z[4 * E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const uint4 v = gload_nt<uint4>(d_planes + poff[j] + e0);
                p[4 * j] = v.x; p[4 * j + 1] = v.y; p[4 * j + 2] = v.z; p[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int d = 0; d < 4 * E; ++d) z[d] = merge_dword<E>(p, d);
            zz_unfold<E, 4 * E>(z);
            s += sum_of<E, 4 * E>(z);
        }
        s = wave_reduce_add<T>(s);
        if (lane_id() == 0) wsum[wave_id()] = s;
        lds_barrier();
        if (threadIdx.x == 0) sums[wk.t] = (u64)(T)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        lds_barrier();                               // the workgroup's next tile writes the wave sums
    }
}

// launch 2: one workgroup a block (grid-stride): the sums of the block's ceil(d_n[b] / tile) tiles -> their exclusive prefixes,
// in place, 256 at a time with a carried total; the next 256 are asked for before the scan of these
__global__ __launch_bounds__(TP_THREADS) void planes_diff_scan(const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                               const u64 *__restrict__ d_n, u64 *__restrict__ sums)
{
    __shared__ u64 wt[2 * (TP_THREADS / 64)];
    u32 turn = 0;
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_n[b];
        if (n > cap[b]) continue;                    // (uniform) past its capacity: its tiles are read by nobody
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        u64 *s = sums + tbase[b];
        u64 carry = 0;
        u64 v = threadIdx.x < nt ? gload<u64>(s + threadIdx.x) : 0;
        for (u32 at = 0; at < nt; at += TP_THREADS) {                          // (uniform)
            const u32 i = at + threadIdx.x;
            const u64 nx = i + TP_THREADS < nt ? gload<u64>(s + i + TP_THREADS) : 0;
            const u64 pre = wg_excl_scan<u64>(v, carry, wt, turn);
            if (i < nt) gstore<u64>(s + i, pre);
            v = nx;
        }
    }
}

template <int E, int Q>
__device__ __forceinline__ void merge_tile_diff(const TpWalk &wk, u32 sh, u32 r, const u8 *d_planes, const u64 *poff,
                                                typename DiffT<E>::T carry, typename DiffT<E>::T *wt, u32 &turn)
{
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u64 e0p = wk.pos0 + (u64)u * PL_PASS;
        if (e0p >= wk.n) break;                      // (WORKGROUP uniform, unlike merge_tile's skip: a barrier is behind it)
        merge_unit<E, Q, false, true>((u8 *)wk.in, wk.n, e0p + (u64)threadIdx.x * PL_UNIT, sh, r, nullptr, d_planes, poff, &carry,
                                      wt, &turn);
    }
}

// launch 3: sums[t] is by now the sum of the d's of the block's tiles in front of tile t
template <int E, bool SKIP = false>
__global__ __launch_bounds__(TP_THREADS) void planes_merge_diff(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                int nblk, const u64 *__restrict__ d_n,
                                                                const u8 *__restrict__ d_planes, const u64 *__restrict__ d_poff,
                                                                int *__restrict__ err, u32 n_tiles, u32 per_wg,
                                                                const u64 *__restrict__ sums, const u64 *__restrict__ d_skip)
{
    using T = typename DiffT<E>::T;
    __shared__ T wt[2 * (TP_THREADS / 64)];
    u32 turn = 0;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (SKIP && d_skip[wk.b]) continue;          // (uniform)
        const u64 *poff = d_poff + (u64)wk.b * E;
        const T carry = (T)sums[wk.t];
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), m = (16u - sh) & 15u, r = m & 3u;
        switch (sh == 0 ? 4u : m >> 2) {             // uniform
        case 0: merge_tile_diff<E, 0>(wk, sh, r, d_planes, poff, carry, wt, turn); break;
        case 1: merge_tile_diff<E, 1>(wk, sh, r, d_planes, poff, carry, wt, turn); break;
        case 2: merge_tile_diff<E, 2>(wk, sh, r, d_planes, poff, carry, wt, turn); break;
        case 3: merge_tile_diff<E, 3>(wk, sh, r, d_planes, poff, carry, wt, turn); break;
        default: merge_tile_diff<E, 4>(wk, sh, r, d_planes, poff, carry, wt, turn); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// the launches read tile_setup's workspace: extra 0 the plane offsets, extra 1 (the XOR kernels: non-NULL) the base offsets,
// the scratch (the merge of differences) the tile sums
template <int E>
void planes_launch(bool merge, const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n, u8 *d_planes, int *err,
                   const u8 *d_base)
{
    const u64 *poff = (const u64 *)a.extra[0], *boff = (const u64 *)a.extra[1];
    if (merge)
        hipLaunchKernelGGL((boff ? planes_merge<E, true> : planes_merge<E, false>), dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off,
                           a.cap, a.tbase, nblk, d_n, (const u8 *)d_planes, poff, err, a.nt, a.per_wg, d_base, boff);
    else
        hipLaunchKernelGGL((boff ? planes_split<E, true> : planes_split<E, false>), dim3(a.wgs), dim3(TP_THREADS), 0, st,
                           (const u8 *)d_el, a.off, a.cap, a.tbase, nblk, d_n, d_planes, poff, err, a.nt, a.per_wg, d_base, boff);
}

// the three launches of the merge of differences; d_skip (the grid merge): the blocks it leaves alone
template <int E, bool SKIP>
void planes_diff_merge_launch(const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n, const u8 *d_planes, int *err,
                              const u64 *d_skip)
{
    const u64 *poff = (const u64 *)a.extra[0];
    u64 *sums = (u64 *)a.scratch;
    if (a.nt)
        hipLaunchKernelGGL((planes_diff_sums<E, SKIP>), dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase,
                           nblk, d_n, d_planes, poff, a.nt, a.per_wg, sums, d_skip);
    const u32 bw = (u32)nblk < TP_MAX_BLOCK_WGS ? (u32)nblk : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(planes_diff_scan, dim3(bw), dim3(TP_THREADS), 0, st, a.cap, a.tbase, nblk, d_n, sums);
    hipLaunchKernelGGL((planes_merge_diff<E, SKIP>), dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblk, d_n,
                       d_planes, poff, err, a.nt, a.per_wg, (const u64 *)sums, d_skip);
}

template <int E>
void planes_diff_launch(bool merge, const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n, u8 *d_planes, int *err)
{
    const u64 *poff = (const u64 *)a.extra[0];
    if (!merge) {
        hipLaunchKernelGGL(planes_split_diff<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblk,
                           d_n, d_planes, poff, err, a.nt, a.per_wg);
        return;
    }
    planes_diff_merge_launch<E, false>(a, st, d_el, nblk, d_n, d_planes, err, nullptr);
}

}  // namespace

// the launch arguments every entry shares.  workspace: tile_setup's with the plane offsets (elem a block) and, with h_base_off,
// the base offsets as extras; scratch, with `sums`: 8 bytes per tile of the capacities that the kernels fill.  The caller has
// checked the arguments.
static int planes_setup(Batch *bt, hipStream_t st, int nblocks, u32 elem, const u64 *h_off, const u64 *h_cap,
                        const u64 *h_plane_off, const u64 *h_base_off, bool sums, TileSetup &a)
{
    const TileExtra x[2] = {{h_plane_off, (size_t)nblocks * elem * 8}, {h_base_off, (size_t)nblocks * 8}};
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, x, h_base_off ? 2 : 1, sums ? 8 : 0, 0, &a)) return rc;
    if (!a.wgs) a.wgs = 1;                           // without a tile one workgroup still looks for blocks past a capacity of 0
    return SHAFA_SUCCESS;
}

// h_base_off (and d_base) non-NULL: the XOR kernels
int planes_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off, const u64 *h_cap,
                      const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, const u8 *d_base, const u64 *h_base_off)
{
    TileSetup a;
    if (int rc = planes_setup(bt, st, nblocks, elem, h_off, h_cap, h_plane_off, h_base_off, false, a)) return rc;
    switch (elem) {
    case 1: planes_launch<1>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err, d_base); break;
    case 2: planes_launch<2>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err, d_base); break;
    case 4: planes_launch<4>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err, d_base); break;
    default: planes_launch<8>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err, d_base); break;
    }
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// the _diff entries: split is one launch; merge is the tile sums (where there is a tile), the blocks' scans and the merge itself
int planes_diff_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                           const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off)
{
    TileSetup a;
    if (int rc = planes_setup(bt, st, nblocks, elem, h_off, h_cap, h_plane_off, nullptr, merge, a)) return rc;
    switch (elem) {
    case 1: planes_diff_launch<1>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 2: planes_diff_launch<2>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 4: planes_diff_launch<4>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    default: planes_diff_launch<8>(merge, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    }
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// the merge of differences as the grid merge's first pass (planes_lag.hip) on that launcher's set-up: extra 0 the plane offsets,
// 8 bytes of scratch or more per tile; the blocks with d_skip[b] != 0 are left to the lag family
void planes_diff_merge_enqueue(u32 elem, const TileSetup &a, hipStream_t st, u8 *d_el, int nblocks, const u64 *d_n,
                               const u8 *d_planes, int *err, const u64 *d_skip)
{
    switch (elem) {
    case 1: planes_diff_merge_launch<1, true>(a, st, d_el, nblocks, d_n, d_planes, err, d_skip); break;
    case 2: planes_diff_merge_launch<2, true>(a, st, d_el, nblocks, d_n, d_planes, err, d_skip); break;
    case 4: planes_diff_merge_launch<4, true>(a, st, d_el, nblocks, d_n, d_planes, err, d_skip); break;
    default: planes_diff_merge_launch<8, true>(a, st, d_el, nblocks, d_n, d_planes, err, d_skip); break;
    }
}
