// seek.hip — a seek index over a file set's blocks (shafa_hipd_seek_index_dev) and the ranged decoder that reads byte ranges
// through it (shafa_hipd_read_spans_dev).  The format of a checkpoint is include/shafa_hip.h's ("Seek index").
//
// A .shaf has no sync markers and an RLE triple may straddle any boundary, so a decoder can only start where something has
// told it the bit offset, the RLE state and the decoded offset.  A checkpoint says exactly that for the position in front of
// symbol k * span of a block's SF-decoded bytes.  Building the index is two launches in which no workgroup waits for another
// and no atomic is used (the result does not depend on scheduling):
//   seek_spans    one wave per span of a block's SF-decoded bytes -> one 16-byte record {code bits of the span, the RLE map
//                 of the span (rld_fsm.hpp), what it adds to the decoded offset per entry state}: rle_measure.hip's monoid
//                     (A then B).map = fn_compose(A.map, B.map)      (A then B).sum[s] = A.sum[s] + B.sum[A.map(s)]
//                 with the bits as a plain sum.  A lane walks span / 64 bytes (4 .. 128), an ordered reduction joins the lanes.
//   seek_blocks   one workgroup per block: an exclusive scan of the block's records in order (a run per thread, the wave, the
//                 four waves), entered in S0 with 0 bits and 0 bytes; every thread then walks its run again and writes the
//                 checkpoints.  Thread 0 leaves the block's decoded size and judges the stream's end as the size pass does.
// Reading is one launch:
//   read_spans    a workgroup is ONE wave whose 64 lanes each own a span of the same block.  The wave first builds the
//                 block's decoding tables in LDS from its shafa_code_table: the codes sorted by their left-aligned value (a
//                 window matches the largest code value not above it, or none: true of any prefix-free code), and a
//                 1024-entry look-up by the window's top 10 bits whose entry is {symbol, length} for codes of <= 10 bits and
//                 "search" otherwise.  Then rounds: every lane SF-decodes up to 64 symbols of its span into its row of LDS
//                 (a table walk is bound by LDS latency: 64 independent walks a wave hide it); the wave then takes the rows
//                 one after the other — lane j the row's symbol j — runs the RLE machine over the row as a scan of maps,
//                 places every symbol's output with an add-scan, and stores the bytes whose decoded offset lies in
//                 [lo, hi): literals one per lane side by side, a run by all lanes together.
// Bounds: a payload byte is only read at an index below the payload's size (an aligned word when it lies wholly inside it,
// single bytes otherwise; bits behind the end read as 0 and a walk that uses one is an error); an output byte is only
// stored when its offset o satisfies lo <= o < hi, at d_out + dst + (o - lo).  The walk of a span is at most `span` symbols.
#include "common.hpp"
#include "internal.hpp"
#include "rld_fsm.hpp"
#include "tile_pass.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int SK_THREADS = 256;                    // the index kernels: four waves
constexpr u32 SK_MAX_WGS = 1u << 16;               // seek_spans: workgroups per launch (grid-stride over the spans)
constexpr u64 SK_BITS_MASK = (1ull << 48) - 1;

// ---- the summary of a piece of a block: rle_measure.hip's, plus the code bits and "a symbol without a code occurred" ----
struct SkAgg {
    u32 f;                                         // map; bit 31: a symbol without a code
    u64 s[3];
    u64 bits;
};
__device__ __forceinline__ SkAgg sk_identity() { return {FN_IDENT, {0, 0, 0}, 0}; }
__device__ __forceinline__ SkAgg sk_then(const SkAgg &a, const SkAgg &b)
{
    SkAgg r;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const u32 m = fn_apply(a.f, (u32)e);
        r.s[e] = a.s[e] + (m == 0 ? b.s[0] : m == 1 ? b.s[1] : b.s[2]);
    }
    r.f = fn_compose(a.f & 63u, b.f & 63u) | ((a.f | b.f) & 0x80000000u);
    r.bits = a.bits + b.bits;
    return r;
}
__device__ __forceinline__ SkAgg sk_shfl_down(const SkAgg &a, int d)
{
    SkAgg o;
    o.f = (u32)__shfl_down((int)a.f, d, 64);
#pragma unroll
    for (int e = 0; e < 3; ++e) o.s[e] = (u64)__shfl_down((unsigned long long)a.s[e], d, 64);
    o.bits = (u64)__shfl_down((unsigned long long)a.bits, d, 64);
    return o;
}
__device__ __forceinline__ SkAgg sk_shfl_up(const SkAgg &a, int d)
{
    SkAgg o;
    o.f = (u32)__shfl_up((int)a.f, d, 64);
#pragma unroll
    for (int e = 0; e < 3; ++e) o.s[e] = (u64)__shfl_up((unsigned long long)a.s[e], d, 64);
    o.bits = (u64)__shfl_up((unsigned long long)a.bits, d, 64);
    return o;
}
// a span's record: {bits (< 2^19) | map << 24 | no-code << 31, sum[S0], sum[S1], sum[S2]} (a span adds < 2^21 bytes)
__device__ __forceinline__ SkAgg sk_read(const uint4 &v)
{
    return {((v.x >> 24) & 63u) | (v.x & 0x80000000u), {v.y, v.z, v.w}, v.x & 0xFFFFFFu};
}

// ---- seek_spans: one wave per span -------------------------------------------------------------------------------------
__global__ __launch_bounds__(SK_THREADS) void seek_spans(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                         const u64 *__restrict__ in_cap, const u32 *__restrict__ sbase, int nblk,
                                                         const u64 *__restrict__ d_in_n, const shafa_code_table *__restrict__ tabs,
                                                         u32 span, int flags, uint4 *__restrict__ rec, u32 n_spans)
{
    const int lane = lane_id();
    const bool sf = (flags & SHAFA_SEEK_SF) != 0, rle = (flags & SHAFA_SEEK_RLE) != 0;
    const u32 piece = span / 64;                                       // 4 .. 128 bytes a lane, a multiple of 4
    const u32 waves = gridDim.x * (SK_THREADS / 64);
    for (u32 g = blockIdx.x * (SK_THREADS / 64) + (u32)wave_id(); g < n_spans; g += waves) {      // (uniform per wave)
        const int b = tp_find_block(sbase, nblk, g);
        u64 n = d_in_n[b];
        if (n > in_cap[b]) n = 0;                                      // SHAFA_OUTSIDE_MODULE, reported by seek_blocks
        const u64 pos0 = (u64)(g - sbase[b]) * span;
        if (pos0 >= n) continue;                                       // no record is read there
        const u8 *in = d_in + in_off[b];
        const u8 *len = tabs ? tabs[b].len : nullptr;
        const u64 p = pos0 + (u64)lane * piece;
        u32 bits = 0, nocode = 0, st[3] = {0, 1, 2}, sum[3] = {0, 0, 0};
        for (u32 q = 0; q < piece; q += 4) {
            if (p + q >= n) break;
            const u32 nv = p + q + 4 <= n ? 4u : (u32)(n - (p + q));
            u32 w = 0;
            if (nv == 4) w = gload<u32>(in + p + q);
            else
                for (u32 j = 0; j < nv; ++j) w |= (u32)gload<u8>(in + p + q + j) << (8 * j);
            for (u32 j = 0; j < nv; ++j) {
                const u32 v = (w >> (8 * j)) & 255u;
                const u32 L = sf ? (u32)gload<u8>(len + v) : 8u;
                bits += L;
                nocode |= (u32)(L == 0);
                if (rle) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        if (st[e] == 0) { if (v) ++sum[e]; else st[e] = 1; }
                        else if (st[e] == 1) st[e] = 2;
                        else { sum[e] += v ? v : 1u; st[e] = 0; }
                    }
                } else ++sum[0];
            }
        }
        if (!rle) sum[1] = sum[2] = sum[0];
        SkAgg a = {rle ? (st[0] | (st[1] << 2) | (st[2] << 4)) | (nocode << 31) : FN_IDENT | (nocode << 31),
                   {sum[0], sum[1], sum[2]}, bits};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const SkAgg o = sk_shfl_down(a, d);
            if (lane + d < 64) a = sk_then(a, o);
        }
        if (lane == 0)
            gstore<uint4>(rec + g, make_uint4((u32)a.bits | ((a.f & 63u) << 24) | (a.f & 0x80000000u), (u32)a.s[0], (u32)a.s[1],
                                              (u32)a.s[2]));
    }
}

// ---- seek_blocks: one workgroup per block ------------------------------------------------------------------------------
__global__ __launch_bounds__(SK_THREADS) void seek_blocks(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                          const u64 *__restrict__ in_cap, const u32 *__restrict__ sbase, int nblk,
                                                          const u64 *__restrict__ d_in_n, const shafa_code_table *__restrict__ tabs,
                                                          u32 span, int flags, const uint4 *__restrict__ rec,
                                                          const u64 *__restrict__ ck_first, u64 *__restrict__ d_ckpt,
                                                          u32 *__restrict__ d_status, u64 *__restrict__ d_out_n, int *__restrict__ err)
{
    __shared__ u32 w_f[4];
    __shared__ u64 w_s[4][3], w_bits[4];
    __shared__ u32 w_long[4];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const bool sf = (flags & SHAFA_SEEK_SF) != 0, rle = (flags & SHAFA_SEEK_RLE) != 0;
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        u64 *ck = d_ckpt + 2 * ck_first[b];
        const u64 n = d_in_n[b];
        if (n > in_cap[b] || n == 0) {                                 // (uniform) refused, or the empty block: checkpoint 0
            if (tid == 0) {
                if (n) set_error(err + b, SHAFA_OUTSIDE_MODULE);
                ck[0] = 0; ck[1] = 0;
                d_status[b] = 0;
                d_out_n[b] = 0;
            }
            continue;
        }
        const u8 *in = d_in + in_off[b];
        const u32 ns = (u32)((n + span - 1) / span);
        const uint4 *r = rec + sbase[b];
        const u32 per = (ns + SK_THREADS - 1) / SK_THREADS;
        const u32 lo = (u32)tid * per < ns ? (u32)tid * per : ns, hi = lo + per < ns ? lo + per : ns;
        SkAgg a = sk_identity();
        for (u32 j = lo; j < hi; ++j) a = sk_then(a, sk_read(gload<uint4>(r + j)));
        // inclusive scan over the wave, in order
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const SkAgg o = sk_shfl_up(a, d);
            if (lane >= d) a = sk_then(o, a);
        }
        const bool too_long = sf && __any(tabs[b].len[tid] > 32) != 0;
        if (lane == 63) {
            w_f[wv] = a.f;
            w_s[wv][0] = a.s[0]; w_s[wv][1] = a.s[1]; w_s[wv][2] = a.s[2];
            w_bits[wv] = a.bits;
            w_long[wv] = too_long;
        }
        lds_barrier();
        SkAgg pre = sk_shfl_up(a, 1);                                  // the wave's threads before this one
        if (lane == 0) pre = sk_identity();
        SkAgg car = sk_identity(), tot = sk_identity();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const SkAgg w = {w_f[q], {w_s[q][0], w_s[q][1], w_s[q][2]}, w_bits[q]};
            if (q < wv) car = sk_then(car, w);
            tot = sk_then(tot, w);
        }
        pre = sk_then(car, pre);
        const bool unindexed = sf && ((w_long[0] | w_long[1] | w_long[2] | w_long[3]) != 0 || (tot.f >> 31) != 0);
        // the walk again: the block is entered in S0
        u32 state = fn_apply(pre.f & 63u, 0);
        u64 off = pre.s[0], bits = pre.bits;
        for (u32 j = lo; j < hi; ++j) {
            if (!unindexed || j == 0) {
                const u64 pend = state == 2 ? (u64)gload<u8>(in + (u64)j * span - 1) : 0ull;
                ck[2 * (u64)j] = (bits & SK_BITS_MASK) | (pend << 48) | ((u64)state << 56);
                ck[2 * (u64)j + 1] = off;
            }
            const uint4 v = gload<uint4>(r + j);
            off += state == 0 ? v.y : state == 1 ? v.z : v.w;
            state = fn_apply((v.x >> 24) & 63u, state);
            bits += v.x & 0xFFFFFFu;
        }
        if (tid == 0) {
            const u32 exit_state = fn_apply(tot.f & 63u, 0);
            const bool bad = rle && (exit_state != 0 || tot.s[0] > (u64)SHAFA_RLE_DECODE_MAX);
            if (bad) set_error(err + b, SHAFA_FILE_UNRECOGNIZABLE);
            d_out_n[b] = bad ? 0 : tot.s[0];
            d_status[b] = unindexed ? SHAFA_SEEK_UNINDEXED : 0u;
        }
        lds_barrier();                                                 // the next block of this workgroup writes the wave results
    }
}

// ---- read_spans --------------------------------------------------------------------------------------------------------
constexpr int RS_LANES = 64;                       // a workgroup is one wave: a span per lane
constexpr int RS_CHUNK = 64;                       // symbols a lane stages per round
constexpr int RS_ROW = RS_CHUNK + 4;               // a row's bytes: 17 words, so that the lanes' rows start in different banks
constexpr int RS_LUT_BITS = 10;
constexpr u64 RS_NO_TASK = ~0ull;

struct RsItem {
    u64 lo, hi, dst;
    u32 block, pad;
};

struct RsShared {
    u32 key[256];                                  // a symbol's code, left aligned
    u32 skey[256];                                 // the codes in ascending order
    u16 ssl[256];                                  // symbol | length << 8, in that order
    u16 lut[1 << RS_LUT_BITS];                     // symbol | length << 8 by the window's top bits; length 0: search
    u8 len[256];
    u8 rows[RS_LANES][RS_ROW];
};

__device__ __forceinline__ u64 rs_readlane64(u64 v, int l)
{
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// bytes [i, i + nb) of a payload of n bytes at p as one big-endian number in the top of 32 bits; bytes at or behind n are 0
// and are not read.  The aligned form is taken only for a whole word inside the payload.
__device__ __forceinline__ u32 rs_load_be(const u8 *p, u64 n, u64 i, u32 nb)
{
    if (nb == 4 && i + 4 <= n && (((uintptr_t)p + i) & 3u) == 0) return bswap32(gload<u32>(p + i));
    u32 v = 0;
    for (u32 j = 0; j < nb; ++j)
        if (i + j < n) v |= (u32)gload<u8>(p + i + j) << (24 - 8 * j);
    return v;
}

__global__ __launch_bounds__(RS_LANES) void read_spans(const u8 *__restrict__ d_file, const u64 *__restrict__ pay_off,
                                                       const u64 *__restrict__ pay_n, const u64 *__restrict__ n_sym,
                                                       const u64 *__restrict__ ck_first, const shafa_code_table *__restrict__ tabs,
                                                       u32 span, int flags, const u64 *__restrict__ d_ckpt,
                                                       const RsItem *__restrict__ items, const u64 *__restrict__ tasks,
                                                       u8 *__restrict__ d_out, int *__restrict__ err)
{
    __shared__ __attribute__((aligned(16))) RsShared sh;
    const int lane = lane_id();
    const bool sf = (flags & SHAFA_SEEK_SF) != 0, rle = (flags & SHAFA_SEEK_RLE) != 0;
    const u64 task = tasks[(u64)blockIdx.x * RS_LANES + lane];
    bool active = task != RS_NO_TASK;
    // lane 0 always has a task; every task of the workgroup lies in its block
    const u32 item0 = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(task >> 32));
    const int b = (int)items[item0].block;
    const RsItem it = items[active ? (u32)(task >> 32) : item0];
    int *my_err = err + (active ? (u32)(task >> 32) : item0);

    // ---- the block's decoding tables --------------------------------------------------------------------------------
    u32 ncodes = 0;
    if (sf) {
        const shafa_code_table &t = tabs[b];
        u32 myL[4], myK[4];
        bool too_long = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32 s = (u32)lane + 64u * q;
            const u32 L = t.len[s];
            const u32 be = bswap32(gload<u32>(t.bits[s]));
            too_long |= L > 32;
            myL[q] = L;
            myK[q] = L == 0 ? 0u : L >= 32 ? be : be & (~0u << (32 - L));
            sh.key[s] = myK[q];
            sh.len[s] = (u8)L;
        }
        if (__any(too_long)) {                                         // (uniform) a block the index marks unindexed
            if (active) set_error(my_err, SHAFA_OUTSIDE_MODULE);
            return;
        }
        lds_barrier();
        u32 mine = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!myL[q]) continue;
            const u32 s = (u32)lane + 64u * q;
            u32 r = 0;
            for (u32 o = 0; o < 256; ++o) {
                const u32 ol = sh.len[o], ok = sh.key[o];
                r += ol != 0 && (ok < myK[q] || (ok == myK[q] && (ol < myL[q] || (ol == myL[q] && o < s))));
            }
            sh.skey[r] = myK[q];
            sh.ssl[r] = (u16)(s | (myL[q] << 8));
            ++mine;
        }
        ncodes = (u32)__builtin_amdgcn_readlane((int)dpp_scan_add(mine), 63);
        lds_barrier();
        for (u32 i = (u32)lane; i < (1u << RS_LUT_BITS); i += RS_LANES) {
            const u32 w = i << (32 - RS_LUT_BITS);
            u32 e = 0;
            if (ncodes && sh.skey[0] <= w) {
                u32 lo = 0, hi = ncodes;
                while (hi - lo > 1) {
                    const u32 mid = (lo + hi) >> 1;
                    if (sh.skey[mid] <= w) lo = mid; else hi = mid;
                }
                const u32 c = sh.ssl[lo], L = c >> 8;
                if (L <= (u32)RS_LUT_BITS && ((w ^ sh.skey[lo]) >> (32 - L)) == 0) e = c;
            }
            sh.lut[i] = (u16)e;
        }
    } else {
        for (u32 i = (u32)lane; i < (1u << RS_LUT_BITS); i += RS_LANES) sh.lut[i] = (u16)((i >> (RS_LUT_BITS - 8)) | (8u << 8));
    }
    lds_barrier();

    // ---- the lane's span --------------------------------------------------------------------------------------------
    const u8 *pay = d_file + pay_off[b];
    const u64 pn = pay_n[b], end_bits = 8 * pn, nsym = n_sym[b];
    const u32 k = (u32)task;
    u64 bitpos = 0, cur = 0, buf = 0, bp = 0;
    u32 state = 0, pend = 0, rem = 0, nxt = 0;
    int avail = 0;
    bool fail = false;
    if (active) {
        const u64 *ck = d_ckpt + 2 * (ck_first[b] + k);
        const u64 w0 = ck[0];
        bitpos = w0 & SK_BITS_MASK;
        pend = (u32)(w0 >> 48) & 255u;
        state = rle ? (u32)(w0 >> 56) & 3u : 0u;
        cur = ck[1];
        const u64 first = (u64)k * span;
        rem = first < nsym ? (u32)(nsym - first < span ? nsym - first : span) : 0u;
        if (state == 3 || bitpos > end_bits) fail = true;
        else if (rem == 0 || cur >= it.hi) active = false;
        else {
            const u64 i0 = bitpos >> 3;
            const u32 r = (u32)bitpos & 7u;
            const u32 nb = 4u - (u32)(((uintptr_t)pay + i0) & 3u);       // 1 .. 4 bytes: the words behind them are aligned
            buf = (u64)rs_load_be(pay, pn, i0, nb) << 32;
            avail = (int)(8 * nb) - (int)r;
            buf <<= r;
            bp = i0 + nb;
            buf |= (u64)rs_load_be(pay, pn, bp, 4) << (32 - avail);
            avail += 32;
            bp += 4;
            nxt = rs_load_be(pay, pn, bp, 4);
        }
        if (fail) { set_error(my_err, SHAFA_FILE_UNRECOGNIZABLE); active = false; }
    }

    while (__any(active)) {
        // ---- phase A: up to RS_CHUNK symbols of the lane's span into its row ----------------------------------------
        u32 cnt = 0;
        if (active) {
            const u32 want = rem < (u32)RS_CHUNK ? rem : (u32)RS_CHUNK;
            u8 *row = sh.rows[lane];
            for (; cnt < want; ++cnt) {
                const u32 win = (u32)(buf >> 32);
                u32 e = sh.lut[win >> (32 - RS_LUT_BITS)], L = e >> 8;
                if (L == 0) {                                          // a code of more than RS_LUT_BITS bits, or none
                    if (!ncodes || sh.skey[0] > win) { fail = true; break; }
                    u32 lo = 0, hi = ncodes;
                    while (hi - lo > 1) {
                        const u32 mid = (lo + hi) >> 1;
                        if (sh.skey[mid] <= win) lo = mid; else hi = mid;
                    }
                    e = sh.ssl[lo];
                    L = e >> 8;
                    if (((win ^ sh.skey[lo]) >> (32 - L)) != 0) { fail = true; break; }    // the window matches no code
                }
                bitpos += L;
                if (bitpos > end_bits) { fail = true; break; }         // a walk past the payload's end
                row[cnt] = (u8)e;
                buf <<= L;
                avail -= (int)L;
                if (avail <= 32) {
                    buf |= (u64)nxt << (32 - avail);
                    avail += 32;
                    bp += 4;
                    nxt = rs_load_be(pay, pn, bp, 4);
                }
            }
            if (fail) {                                                // nothing more is written for this span
                set_error(my_err, SHAFA_FILE_UNRECOGNIZABLE);
                active = false;
                cnt = 0;
            }
            rem -= cnt;
        }
        lds_barrier();
        // ---- phase B: the rows one after the other, lane j the row's symbol j ---------------------------------------
        for (u64 rows = __ballot(cnt > 0); rows; rows &= rows - 1) {
            const int r = __builtin_ctzll(rows);                       // (uniform)
            const u32 c = (u32)__builtin_amdgcn_readlane((int)cnt, r);
            const u64 cu = rs_readlane64(cur, r), lo = rs_readlane64(it.lo, r), hi = rs_readlane64(it.hi, r);
            u8 *dst = d_out + rs_readlane64(it.dst, r);
            const u32 sym = (u32)lane < c ? sh.rows[r][lane] : 0u;
            u64 ncur;
            u32 nstate = 0, npend = 0;
            if (!rle) {
                const u64 o = cu + (u32)lane;
                if ((u32)lane < c && o >= lo && o < hi) gstore<u8>(dst + (o - lo), (u8)sym);
                ncur = cu + c;
            } else {
                const u32 st0 = (u32)__builtin_amdgcn_readlane((int)state, r), pd = (u32)__builtin_amdgcn_readlane((int)pend, r);
                u32 f = (u32)lane < c ? ((sym == 0 ? 1u : 0u) | (2u << 2)) : FN_IDENT;      // S0: escape or literal; S1 -> S2 -> S0
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const u32 y = (u32)__shfl_up((int)f, d, 64);
                    if (lane >= d) f = fn_compose(y, f);
                }
                u32 fex = (u32)__shfl_up((int)f, 1, 64), prev = (u32)__shfl_up((int)sym, 1, 64);
                if (lane == 0) { fex = FN_IDENT; prev = pd; }
                const u32 es = fn_apply(fex, st0);
                const u32 nout = (u32)lane < c ? (es == 0 ? (u32)(sym != 0) : es == 2 ? (sym ? sym : 1u) : 0u) : 0u;
                const u32 val = es == 2 ? prev : sym;
                const u32 incl = dpp_scan_add(nout);
                const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                const u64 o = cu + (incl - nout);
                if (cu + total > lo && cu < hi) {                      // (uniform) the row touches the range
                    if (nout == 1 && o >= lo && o < hi) gstore<u8>(dst + (o - lo), (u8)val);
                    for (u64 runs = __ballot(nout > 1); runs; runs &= runs - 1) {
                        const int q = __builtin_ctzll(runs);
                        const u64 s0 = rs_readlane64(o, q);
                        const u32 ln = (u32)__builtin_amdgcn_readlane((int)nout, q);     // <= 255
                        const u32 v = (u32)__builtin_amdgcn_readlane((int)val, q);
                        for (u32 i = (u32)lane; i < ln; i += RS_LANES) {
                            const u64 x = s0 + i;
                            if (x >= lo && x < hi) gstore<u8>(dst + (x - lo), (u8)v);
                        }
                    }
                }
                ncur = cu + total;
                nstate = fn_apply((u32)__builtin_amdgcn_readlane((int)f, 63), st0);
                npend = (u32)__builtin_amdgcn_readlane((int)sym, (int)c - 1);
            }
            if (lane == r) { cur = ncur; state = nstate; pend = npend; }
        }
        // ---- the end of a span: it agrees with the next checkpoint, or it ends the block outside a triple ------------
        if (active && rem == 0) {
            const u64 nck = nsym ? (nsym + span - 1) / span : 1;
            bool bad;
            if ((u64)k + 1 < nck) {
                const u64 *nx = d_ckpt + 2 * (ck_first[b] + k + 1);
                const u64 w0 = nx[0];
                bad = (w0 & SK_BITS_MASK) != bitpos || nx[1] != cur || (rle && ((u32)(w0 >> 56) & 3u) != state);
            } else bad = rle && state != 0;
            if (bad) set_error(my_err, SHAFA_FILE_UNRECOGNIZABLE);
            active = false;
        }
        if (active && cur >= it.hi) active = false;                    // nothing behind here lies in the range
        lds_barrier();                                                 // the next round overwrites the rows
    }
}

}  // namespace

// workspace: tile_setup's with the span as the tile and one extra, the first checkpoints; scratch: the records, 16 B per span
// of the capacities.  The grids are SK_*'s.
int seek_index_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                          const u64 *d_in_n, const shafa_code_table *d_tables, u32 span, int flags, const u64 *h_ckpt_first,
                          u64 *d_ckpt, u32 *d_status, u64 *d_out_n)
{
    const TileExtra x = {h_ckpt_first, (size_t)nblocks * 8};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_in_off, h_in_cap, span, &x, 1, 16, 0, &a)) return rc;
    const u64 *d_ck = (const u64 *)a.extra[0];
    if (a.nt) {
        const u64 want = ceil_div_u64(a.nt, SK_THREADS / 64);
        hipLaunchKernelGGL(seek_spans, dim3((u32)(want < SK_MAX_WGS ? want : SK_MAX_WGS)), dim3(SK_THREADS), 0, st, d_in, a.off,
                           a.cap, a.tbase, nblocks, d_in_n, d_tables, span, flags, (uint4 *)a.scratch, a.nt);
    }
    hipLaunchKernelGGL(seek_blocks, dim3((u32)nblocks < SK_MAX_WGS ? (u32)nblocks : SK_MAX_WGS), dim3(SK_THREADS), 0, st, d_in,
                       a.off, a.cap, a.tbase, nblocks, d_in_n, d_tables, span, flags, (const uint4 *)a.scratch, d_ck, d_ckpt, d_status,
                       d_out_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// The spans of the items, block after block, 64 to a workgroup; a workgroup's spans lie in one block (the slots left over at
// a change of block hold no task).  workspace, all uploaded: [payload offsets][payload sizes][symbol counts][first
// checkpoints][items][tasks: item << 32 | checkpoint].  The caller has checked every item against its block.
int read_spans_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_file, const u64 *h_pay_off, const u64 *h_pay_n,
                          const u64 *h_n_symbols, const u64 *h_ckpt_first, const shafa_code_table *d_tables, u32 span, int flags,
                          const u64 *d_ckpt, int nitems, const int *h_item_block, const u64 *h_item_first,
                          const u64 *h_item_last, const u64 *h_item_lo, const u64 *h_item_hi, const u64 *h_item_dst, u8 *d_out)
{
    std::vector<int> order;
    order.reserve((size_t)nitems);
    u64 ntasks = 0;
    for (int i = 0; i < nitems; ++i)
        if (h_item_lo[i] < h_item_hi[i]) {
            order.push_back(i);
            ntasks += h_item_last[i] - h_item_first[i] + 1;
        }
    if (order.empty()) return SHAFA_SUCCESS;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_item_block[a] < h_item_block[b]; });
    int changes = 1;
    for (size_t i = 1; i < order.size(); ++i) changes += h_item_block[order[i]] != h_item_block[order[i - 1]];
    const u64 slots_max = ntasks + (u64)changes * (RS_LANES - 1);
    if (slots_max > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    const size_t nb = (size_t)nblocks, ni = (size_t)nitems;
    size_t up_bytes = 0;
    const size_t u_off = take16(up_bytes, nb * 8), u_n = take16(up_bytes, nb * 8), u_sym = take16(up_bytes, nb * 8);
    const size_t u_ck = take16(up_bytes, nb * 8), u_items = take16(up_bytes, ni * sizeof(RsItem));
    const size_t u_tasks = take16(up_bytes, (size_t)((slots_max + RS_LANES - 1) / RS_LANES * RS_LANES) * 8);
    int rc = batch_reserve(bt, st, up_bytes);
    if (rc) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    u8 *hs = (u8 *)batch_stage(bt, st, up_bytes);
    if (!hs) return SHAFA_LACK_OF_MEMORY;
    memset(hs, 0, u_tasks);
    memcpy(hs + u_off, h_pay_off, nb * 8);
    memcpy(hs + u_n, h_pay_n, nb * 8);
    memcpy(hs + u_sym, h_n_symbols, nb * 8);
    memcpy(hs + u_ck, h_ckpt_first, nb * 8);
    RsItem *hi = (RsItem *)(hs + u_items);
    for (int i = 0; i < nitems; ++i) hi[i] = {h_item_lo[i], h_item_hi[i], h_item_dst[i], (u32)h_item_block[i], 0u};
    u64 *ht = (u64 *)(hs + u_tasks);
    u64 nslots = 0;
    int prev_block = -1;
    for (int i : order) {
        if (h_item_block[i] != prev_block)
            while (nslots % RS_LANES) ht[nslots++] = RS_NO_TASK;
        prev_block = h_item_block[i];
        for (u64 k = h_item_first[i]; k <= h_item_last[i]; ++k) ht[nslots++] = ((u64)(u32)i << 32) | (u32)k;
    }
    while (nslots % RS_LANES) ht[nslots++] = RS_NO_TASK;
    const size_t used = (u_tasks + (size_t)nslots * 8 + 15) & ~(size_t)15;
    if ((rc = batch_upload(bt, st, ws, hs, used))) return rc;
    hipLaunchKernelGGL(read_spans, dim3((u32)(nslots / RS_LANES)), dim3(RS_LANES), 0, st, d_file, (const u64 *)(ws + u_off),
                       (const u64 *)(ws + u_n), (const u64 *)(ws + u_sym), (const u64 *)(ws + u_ck), d_tables, span, flags, d_ckpt,
                       (const RsItem *)(ws + u_items), (const u64 *)(ws + u_tasks), d_out, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
