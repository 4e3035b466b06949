// rle_encode_hist.hip — the histogram of a block's RLE bytes without the RLE bytes (shafa_hipd_rle_encoded_hist_dev).
//
// The encoder's rule per maximal run of byte s with length L, q = L / 255, m = L % 255 (f.c:29-55; runs end at the
// block's end): q triples {0, s, 255}; then for m > 0 one triple {0, s, m} if s == 0 or m >= 4, else m literals s.
// Stated as THE PLAIN HISTOGRAM OF THE INPUT PLUS A SIGNED CORRECTION PER ENCODED RUN: a run with s != 0 and L < 4 is m
// literals, i.e. its own bytes — no correction.  Any other run takes L from H[s] and adds the bytes above (charge()).  Wrapping
// arithmetic; every total is exact, and the block's RLE size is the sum of its 256 counts.
// A piece of the input is summarised by {n bytes, first byte, length of its first run, last byte, length of its last run}, as
// in rle_encode_measure.hip; two neighbouring summaries compose associatively (rs_then).  Where that pass adds a run's size to
// `inside`, this one charges the run's correction — so every composition here is done by exactly ONE thread (an aligned tree,
// not tile_pass.hpp's overlapping reduction), and the summary needs no `inside`.
// Two launches, no workgroup ever waits for another:
//   rle_ehist_tiles    every 8 KiB tile: its bytes into a 256 x 32 replicated LDS histogram (hist.hip's layout: a lane's
//                      replica is its bank), the corrections of the runs strictly inside the tile into the same bins, one
//                      16-byte record {n, first byte, first-run length, last byte, last-run length}.  A workgroup walks a run
//                      of consecutive tiles and adds its bins to the block's counts when the block changes and at its end: at
//                      most 256 global atomics each time.  Per workgroup and block the bins are >= 0 (a run is charged where
//                      all of its bytes were counted), so 32-bit bins hold them.
//   rle_ehist_blocks   one workgroup per block composes the records in order (64-bit lengths) and charges what the tiles
//                      could not: the runs that touch a tile border — at most two per tile — and the block's first and last
//                      run, into a 64-bit LDS histogram.  Then counts = the tiles' sums + these, and d_out_n = their sum.
// The summary and its composition are this file's own (rle_encode_measure.hip keeps Rem / rem_then): a shared header would
// have to leave every existing kernel's registers as they are, which DESIGN 7.13 found hard to hold, and the two differ in
// what a composition does.
//
// Algorithmic HBM bytes per block: n read, 16 bytes per 8 KiB tile written and read again, 2 KiB of counts.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr int EH_REP = 32;                         // LDS replicas of the tile kernel's histogram

// the correction of one maximal run: add(bin, wrapping amount)
template <typename T, typename Add>
__device__ __forceinline__ void charge(u32 s, T L, Add &&add)
{
    if (s != 0 && L < 4) return;                    // its own bytes
    const T q = L / 255u;
    const u32 m = (u32)(L - q * 255u);
    add(s, (T)0 - L);
    if (q) {
        add(0u, q);
        add(s, q);
        add(255u, q);
    }
    if (m) {
        if (s == 0 || m >= 4) {
            add(0u, (T)1);
            add(s, (T)1);
            add(m, (T)1);
        } else {
            add(s, (T)m);
        }
    }
}

// n == 0: the empty piece (neutral on both sides); flen == n: one run (then llen == n)
template <typename T>
struct Rs {
    T n, flen, llen;
    u32 fb, lb;
};

// a's piece, then b's: a run that neither piece could still grow is charged here
template <typename T, typename Add>
__device__ __forceinline__ Rs<T> rs_then(const Rs<T> &a, const Rs<T> &b, Add &&add)
{
    if (a.n == 0) return b;
    if (b.n == 0) return a;
    const bool ua = a.flen == a.n, ub = b.flen == b.n;
    Rs<T> r;
    r.n = a.n + b.n;
    r.fb = a.fb;
    r.lb = b.lb;
    r.flen = a.flen;
    r.llen = b.llen;
    if (a.lb == b.fb) {                             // one run crosses the seam
        if (ua) r.flen = a.n + b.flen;              // (both: the whole piece is one run)
        if (ub) r.llen = a.llen + b.n;
        if (!ua && !ub) charge<T>(a.lb, a.llen + b.flen, add);
    } else {
        if (!ua) charge<T>(a.lb, a.llen, add);
        if (!ub) charge<T>(b.fb, b.flen, add);
    }
    return r;
}

template <typename T>
__device__ __forceinline__ Rs<T> rs_from_lane(const Rs<T> &a, int d)
{
    Rs<T> o;
    o.n = (T)__shfl_down(a.n, d, 64);
    o.flen = (T)__shfl_down(a.flen, d, 64);
    o.llen = (T)__shfl_down(a.llen, d, 64);
    const u32 e = (u32)__shfl_down((int)(a.fb | (a.lb << 8)), d, 64);
    o.fb = e & 0xFFu;
    o.lb = e >> 8;
    return o;
}

// The wave's summary in lane 0.  An aligned tree: at distance d the lanes that are multiples of 2 d put their d lanes
// together with the d lanes behind them, so every seam between two lanes is composed — and its runs charged — exactly once.
template <typename T, typename Add>
__device__ __forceinline__ Rs<T> rs_wave_reduce(Rs<T> a, Add &&add)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Rs<T> o = rs_from_lane<T>(a, d);
        if ((lane & (2 * d - 1)) == 0) a = rs_then<T>(a, o, add);
    }
    return a;
}

// byte i of the lane's 32, the words by value: selects between registers (handed over as an array they became a select
// between addresses of a copy in scratch)
__device__ __forceinline__ u32 byte_of(u32 i, u32 w0, u32 w1, u32 w2, u32 w3, u32 w4, u32 w5, u32 w6, u32 w7)
{
    const u32 k = i >> 2;
    u32 lw = w0;
    lw = k == 1u ? w1 : lw;
    lw = k == 2u ? w2 : lw;
    lw = k == 3u ? w3 : lw;
    lw = k == 4u ? w4 : lw;
    lw = k == 5u ? w5 : lw;
    lw = k == 6u ? w6 : lw;
    lw = k == 7u ? w7 : lw;
    return (lw >> (8u * (i & 3u))) & 0xFFu;
}
#define BYTE_AT(w, i) byte_of((i), (w)[0], (w)[1], (w)[2], (w)[3], (w)[4], (w)[5], (w)[6], (w)[7])

__global__ __launch_bounds__(TP_THREADS) void rle_ehist_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                              const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                              int nblk, const u64 *__restrict__ d_in_n,
                                                              uint4 *__restrict__ rec, u32 n_tiles, u32 per_wg,
                                                              u64 *__restrict__ d_freq)
{
    __shared__ u32 h[256 * EH_REP];                 // bin s of replica r at s * 32 + r
    __shared__ __attribute__((aligned(16))) uint4 sh_a[2][4];      // per tile parity and wave: {n, flen, llen, fb | lb << 8}
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const u32 rep = (u32)tid & (EH_REP - 1);
    auto add = [&](u32 bin, u32 v) { atomicAdd(&h[bin * EH_REP + rep], v); };
    // the workgroup's bins -> block b's counts; every thread sums and clears the 32 replicas of bin tid (rotated: no conflicts)
    auto flush = [&](int b) {
        lds_barrier();
        u32 c = 0;
#pragma unroll
        for (int r = 0; r < EH_REP; ++r) {
            u32 *p = &h[tid * EH_REP + ((r + tid) & (EH_REP - 1))];
            c += *p;
            *p = 0;
        }
        if (c) atomicAdd((unsigned long long *)(d_freq + (size_t)b * 256 + tid), (unsigned long long)c);
        lds_barrier();
    };
    for (int i = tid; i < 256 * EH_REP; i += TP_THREADS) h[i] = 0;
    lds_barrier();
    int cur_b = -1;                                 // the block whose counts the bins hold
    u32 turn = 0;
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur_b) {                        // (uniform)
            if (cur_b >= 0) flush(cur_b);
            cur_b = wk.b;
        }
        // ---- the lane's 32 bytes; bytes past the block's end are never loaded ---------------------------------------------
        u32 w[8];
        const u32 nvalid = tp_lane_load(wk.in, wk.pos0, wk.n, w);
        // ---- masks over the lane's bytes: valid, zero, head (first byte, or differs from the byte before) -----------------
        const u32 vm = nvalid >= 32u ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
        u32 x[8];
        x[0] = w[0] ^ (w[0] << 8);
#pragma unroll
        for (int i = 1; i < 8; ++i) x[i] = w[i] ^ __builtin_amdgcn_alignbit(w[i], w[i - 1], 24);
        const u32 Z = zmask32(w) & vm;
        const u32 H = (~zmask32(x) | 1u) & vm;
        // ---- the lane's summary -------------------------------------------------------------------------------------------
        Rs<u32> a;
        a.n = nvalid;
        a.fb = w[0] & 0xFFu;
        a.lb = BYTE_AT(w, (nvalid ? nvalid : 1u) - 1u);
        const u32 H2 = H & ~1u;                     // heads behind the first byte: none when the lane is one run
        const bool one = H2 == 0u;
        const u32 p = H ? 31u - (u32)__builtin_clz(H) : 0u;        // the last head
        a.flen = one ? nvalid : (u32)__builtin_ctz(H2);
        a.llen = nvalid - p;
        // ---- the plain histogram of the lane's bytes ----------------------------------------------------------------------
        if (one) {
            if (nvalid) add(a.fb, nvalid);
        } else if (nvalid == (u32)TP_BPL) {
#pragma unroll
            for (int j = 0; j < TP_BPL; ++j) add((w[j >> 2] >> (8 * (j & 3))) & 0xFFu, 1u);
        } else {
#pragma unroll
            for (int j = 0; j < TP_BPL; ++j)
                if ((u32)j < nvalid) add((w[j >> 2] >> (8 * (j & 3))) & 0xFFu, 1u);
        }
        // ---- the runs strictly inside the lane that are encoded: zeros of any length, others from 4 bytes (the head after
        // such a run lies inside the lane, so the three bits behind a head tell a run of 4 or more) --------------------------
        const u32 I = one ? 0u : (((1u << p) - 1u) & ~((1u << (a.flen & 31u)) - 1u));
        u32 todo = H & I & (Z | ~((H >> 1) | (H >> 2) | (H >> 3)));
        while (todo) {
            const u32 i = (u32)__builtin_ctz(todo);
            todo &= todo - 1u;
            const u32 L = (u32)__builtin_ctz(H >> (i + 1u)) + 1u;
            charge<u32>(BYTE_AT(w, i), L, add);
        }
        // ---- the wave's summary, in lane 0 --------------------------------------------------------------------------------
        if (__all(!one && nvalid == (u32)TP_BPL)) {
            // every lane's first and last run end inside it: the seam with the lane after it is one run of < 64 bytes, or two
            const u32 nx = (u32)__shfl_down((int)(a.fb | (a.flen << 8)), 1, 64);
            const u32 nfb = nx & 0xFFu, nfl = nx >> 8;
            if (lane < 63) {
                if (a.lb == nfb) {
                    charge<u32>(a.lb, a.llen + nfl, add);
                } else {
                    charge<u32>(a.lb, a.llen, add);
                    charge<u32>(nfb, nfl, add);
                }
            }
            a.lb = (u32)__builtin_amdgcn_readlane((int)a.lb, 63);
            a.llen = (u32)__builtin_amdgcn_readlane((int)a.llen, 63);
            a.n = 64u * TP_BPL;                     // lane 0 keeps its own first byte and first run
        } else {
            a = rs_wave_reduce<u32>(a, add);
        }
        uint4 *slot = sh_a[turn & 1u];
        ++turn;
        if (lane == 0) slot[wv] = make_uint4(a.n, a.flen, a.llen, a.fb | (a.lb << 8));
        lds_barrier();
        if (tid == 0) {
            Rs<u32> r = {0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = slot[q];
                const Rs<u32> o = {v.x, v.y, v.z, v.w & 0xFFu, v.w >> 8};
                r = rs_then<u32>(r, o, add);
            }
            gstore<uint4>(rec + wk.t, make_uint4(r.n | (r.fb << 16) | (r.lb << 24), r.flen, r.llen, 0u));
        }
        // the next tile writes the other set of slots; this set is written again after the next tile's barrier, which
        // thread 0 reaches only after it has read these
    }
    if (cur_b >= 0) flush(cur_b);
}

__global__ __launch_bounds__(TP_THREADS) void rle_ehist_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                               int nblk, const u64 *__restrict__ d_in_n,
                                                               const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                                               u64 *d_freq, int *__restrict__ err)
{
    __shared__ unsigned long long bh[256];          // this kernel's corrections, wrapping
    __shared__ u64 ws[4][3];                        // the four wave summaries, then (ws[q][0]) the four wave sums
    __shared__ u32 wb[4];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    auto add = [&](u32 bin, u64 v) { atomicAdd(&bh[bin], (unsigned long long)v); };
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_in_n[b];
        if (n > in_cap[b]) {                        // (uniform) past the block's region: the counts stay 0
            if (tid == 0) {
                set_error(err + b, SHAFA_OUTSIDE_MODULE);
                d_out_n[b] = 0;
            }
            continue;
        }
        bh[tid] = 0;
        lds_barrier();
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        const uint4 *r = rec + tbase[b];
        const u32 per = (nt + TP_THREADS - 1) / TP_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        Rs<u64> a = {0, 0, 0, 0, 0};
        for (u32 j = lo; j < hi; ++j) {
            const uint4 v = gload<uint4>(r + j);
            const Rs<u64> o = {v.x & 0xFFFFu, v.y, v.z, (v.x >> 16) & 0xFFu, v.x >> 24};
            a = rs_then<u64>(a, o, add);
        }
        a = rs_wave_reduce<u64>(a, add);
        if (lane == 0) {
            ws[wv][0] = a.n; ws[wv][1] = a.flen; ws[wv][2] = a.llen;
            wb[wv] = a.fb | (a.lb << 8);
        }
        lds_barrier();
        if (tid == 0) {
            Rs<u64> t = {0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const Rs<u64> o = {ws[q][0], ws[q][1], ws[q][2], wb[q] & 0xFFu, wb[q] >> 8};
                t = rs_then<u64>(t, o, add);
            }
            if (t.n) {                              // the runs that end at the block's ends
                if (t.flen == t.n) {
                    charge<u64>(t.fb, t.n, add);
                } else {
                    charge<u64>(t.fb, t.flen, add);
                    charge<u64>(t.lb, t.llen, add);
                }
            }
        }
        lds_barrier();
        // counts = what the tiles kernel added up (complete: the launch before this one) + this block's corrections
        u64 *f = d_freq + (size_t)b * 256;
        const u64 c = f[tid] + bh[tid];
        f[tid] = c;
        const u64 s = wave_reduce_add<u64>(c);
        if (lane == 0) ws[wv][0] = s;
        lds_barrier();
        if (tid == 0) d_out_n[b] = ws[0][0] + ws[1][0] + ws[2][0] + ws[3][0];
        lds_barrier();                              // the next block of this workgroup writes bh and ws
    }
}

}  // namespace

// workspace: tp_launch's (tile_pass.hpp), with the counts: they are zeroed first, the tiles kernel adds to them.  The grid is
// this launcher's own: a workgroup takes at least a few tiles where the call has many, so that clearing and summing its 32 KiB
// of bins is paid once per several tiles.
int rleehist_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                        const u64 *d_in_n, u64 *d_out_n, u64 *d_freq)
{
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_in_off, h_in_cap, TP_TILE, nullptr, 0, 16, 0, &a)) return rc;
    HIP_TRY(hipMemsetAsync(d_freq, 0, (size_t)nblocks * 256 * sizeof(u64), st));
    if (a.nt) {
        const u32 nt = a.nt, few = (nt + 4095u) / 4096u;
        u32 per_wg = a.per_wg;
        if (per_wg < 8u) per_wg = few < 8u ? (few > per_wg ? few : per_wg) : 8u;
        const u32 wgs = (nt + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(rle_ehist_tiles, dim3(wgs), dim3(TP_THREADS), 0, st, d_in, a.off, a.cap, a.tbase, nblocks, d_in_n,
                           (uint4 *)a.scratch, nt, per_wg, d_freq);
    }
    const u32 bw = (u32)nblocks < TP_MAX_BLOCK_WGS ? (u32)nblocks : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(rle_ehist_blocks, dim3(bw), dim3(TP_THREADS), 0, st, a.cap, a.tbase, nblocks, d_in_n,
                       (const uint4 *)a.scratch, d_out_n, d_freq, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
