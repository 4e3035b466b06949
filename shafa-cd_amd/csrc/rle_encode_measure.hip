// rle_encode_measure.hip — the RLE size of input blocks without encoding them (shafa_hipd_rle_encoded_size_dev).
//
// The encoder's size rule per maximal run of byte s with length L (f.c:29-55; runs end at the block's end):
//     f(s, L) = 3 (L / 255) + g(s, L % 255)       g(s, 0) = 0,  g(s, m) = 3 if s == 0 or m >= 4, else m
// A piece of the input is summarised by {n bytes, first byte, length of its first run, last byte, length of its last run,
// size of the runs strictly inside}; the piece is one run exactly when its first run has n bytes.  Two neighbouring
// summaries compose associatively (rem_then): a run that crosses the seam has its two lengths added before f is applied,
// a run that ends at the seam from either side moves inside.  The block's size is f(first run) + inside + f(last run), or
// f(the whole length) for a block of one run.
// Two launches, no workgroup ever waits for another (no tickets, no descriptors, no agent-scope atomics):
//   rle_esize_tiles    every 8 KiB tile -> one 16-byte record.  A lane summarises its 32 bytes from three masks (equal to
//                      the byte before, zero, valid): a run shorter than 255 costs min(L, 3) when s != 0 — the bytes at most
//                      two places behind a head — and 3 when s == 0, so the runs inside a lane are two popcounts.  A wave
//                      in which no lane is one run (text, records, Zipf bytes) settles every seam with the lane after it and
//                      adds up; any other wave is put together by an ordered reduction of the summaries.
//   rle_esize_blocks   one workgroup per block: each thread composes a run of consecutive records with 64-bit lengths (a
//                      64 MiB block can be one run), an ordered reduction lanes -> waves -> block, thread 0 applies f.
// The tile walk, the lane's load, the ordered reduction, the blocks kernel's skeleton and the launcher are tile_pass.hpp's,
// shared with the decoded-size pass; this file holds the summary.
//
// Algorithmic HBM bytes per block: n read, 16 bytes per 8 KiB tile written and read again.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

// the size of one maximal run
template <typename T>
__device__ __forceinline__ T rem_cost(u32 s, T L)
{
    const T q = L / 255u;
    const u32 m = (u32)(L - q * 255u);
    return 3u * q + (m == 0 ? 0u : (s == 0 || m >= 4) ? 3u : m);
}

// n == 0: the empty piece (neutral on both sides); flen == n: one run (then llen == n and inside == 0)
template <typename T>
struct Rem {
    T n, flen, llen, inside;
    u32 fb, lb;
};

template <typename T>
__device__ __forceinline__ Rem<T> rem_then(const Rem<T> &a, const Rem<T> &b)
{
    if (a.n == 0) return b;
    if (b.n == 0) return a;
    const bool ua = a.flen == a.n, ub = b.flen == b.n;
    Rem<T> r;
    r.n = a.n + b.n;
    r.fb = a.fb;
    r.lb = b.lb;
    r.flen = a.flen;
    r.llen = b.llen;
    r.inside = a.inside + b.inside;
    if (a.lb == b.fb) {                             // one run crosses the seam
        if (ua) r.flen = a.n + b.flen;              // (both: the whole piece is one run)
        if (ub) r.llen = a.llen + b.n;
        if (!ua && !ub) r.inside += rem_cost<T>(a.lb, a.llen + b.flen);
    } else {
        if (!ua) r.inside += rem_cost<T>(a.lb, a.llen);
        if (!ub) r.inside += rem_cost<T>(b.fb, b.flen);
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T rem_size(const Rem<T> &a)
{
    if (a.n == 0) return 0;
    if (a.flen == a.n) return rem_cost<T>(a.fb, a.n);
    return rem_cost<T>(a.fb, a.flen) + a.inside + rem_cost<T>(a.lb, a.llen);
}

// the summary trait of tile_pass.hpp's ordered reduction, with 32-bit lengths inside a tile and 64-bit ones across a block
template <typename T>
struct RemSum {
    using Agg = Rem<T>;
    static __device__ __forceinline__ Agg then(const Agg &a, const Agg &b) { return rem_then<T>(a, b); }
    static __device__ __forceinline__ Agg from_lane(const Agg &a, int d)
    {
        Agg o;
        o.n = (T)__shfl_down(a.n, d, 64);
        o.flen = (T)__shfl_down(a.flen, d, 64);
        o.llen = (T)__shfl_down(a.llen, d, 64);
        o.inside = (T)__shfl_down(a.inside, d, 64);
        const u32 e = (u32)__shfl_down((int)(a.fb | (a.lb << 8)), d, 64);
        o.fb = e & 0xFFu;
        o.lb = e >> 8;
        return o;
    }
};

// a run shorter than 255 bytes
__device__ __forceinline__ u32 res_short_cost(u32 s, u32 L) { return s == 0 ? 3u : (L < 3u ? L : 3u); }

__global__ __launch_bounds__(TP_THREADS) void rle_esize_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                              const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                              int nblk, const u64 *__restrict__ d_in_n,
                                                              uint4 *__restrict__ rec, u32 n_tiles, u32 per_wg)
{
    __shared__ __attribute__((aligned(16))) uint4 sh_a[2][4];      // per tile parity and wave: {n | flen << 16, llen | fb << 16 | lb << 24, inside, -}
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    u32 turn = 0;
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
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
        Rem<u32> a;
        a.n = nvalid;
        a.fb = w[0] & 0xFFu;
        {
            const u32 j = (nvalid ? nvalid : 1u) - 1u;
            u32 lw = w[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) lw = (j >> 2) == (u32)i ? w[i] : lw;
            a.lb = (lw >> (8u * (j & 3u))) & 0xFFu;
        }
        const u32 H2 = H & ~1u;                     // heads behind the first byte: none when the lane is one run
        const bool one = H2 == 0u;
        const u32 p = H ? 31u - (u32)__builtin_clz(H) : 0u;        // the last head
        a.flen = one ? nvalid : (u32)__builtin_ctz(H2);
        a.llen = nvalid - p;
        const u32 I = one ? 0u : (((1u << p) - 1u) & ~((1u << (a.flen & 31u)) - 1u));     // the runs strictly inside the lane
        const u32 near = H | (H << 1) | (H << 2);   // at most two places behind a head
        a.inside = (u32)__builtin_popcount(near & ~Z & I) + 3u * (u32)__builtin_popcount(H & Z & I);

        // ---- the wave's summary, in lane 0 --------------------------------------------------------------------------------
        if (__all(!one && nvalid == (u32)TP_BPL)) {
            // every lane's first and last run end inside it: the seam with the lane after it is one run of < 64 bytes, or two
            const u32 nx = (u32)__shfl_down((int)(a.fb | (a.flen << 8)), 1, 64);
            const u32 nfb = nx & 0xFFu, nfl = nx >> 8;
            u32 c = a.inside;
            if (lane < 63)
                c += a.lb == nfb ? res_short_cost(a.lb, a.llen + nfl) : res_short_cost(a.lb, a.llen) + res_short_cost(nfb, nfl);
            const u32 tot = dpp_scan_add(c);
            a.inside = (u32)__builtin_amdgcn_readlane((int)tot, 63);
            a.lb = (u32)__builtin_amdgcn_readlane((int)a.lb, 63);
            a.llen = (u32)__builtin_amdgcn_readlane((int)a.llen, 63);
            a.n = 64u * TP_BPL;                     // lane 0 keeps its own first byte and first run
        } else {
            a = tp_wave_reduce<RemSum<u32>>(a);
        }
        uint4 *slot = sh_a[turn & 1u];
        ++turn;
        if (lane == 0) slot[wv] = make_uint4(a.n | (a.flen << 16), a.llen | (a.fb << 16) | (a.lb << 24), a.inside, 0u);
        lds_barrier();
        if (tid == 0) {
            Rem<u32> r = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = slot[q];
                const Rem<u32> o = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.z, (v.y >> 16) & 0xFFu, v.y >> 24};
                r = rem_then<u32>(r, o);
            }
            gstore<uint4>(rec + wk.t, make_uint4(r.n | (r.fb << 16) | (r.lb << 24), r.flen, r.llen, r.inside));
        }
        // the next tile writes the other set of slots; this set is written again after the next tile's barrier, which
        // thread 0 reaches only after it has read these
    }
}

// the blocks kernel's four wave results: touched by RemBlockSum's put and finish only, which tp_blocks calls between its two
// barriers
__shared__ u64 rem_ws[4][4];
__shared__ u32 rem_wb[4];

// the blocks kernel's summary
struct RemBlockSum : RemSum<u64> {
    static __device__ __forceinline__ Agg identity() { return {0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ Agg read(const uint4 &v) { return {v.x & 0xFFFFu, v.y, v.z, v.w, (v.x >> 16) & 0xFFu, v.x >> 24}; }
    static __device__ __forceinline__ void put(int q, const Agg &a)
    {
        rem_ws[q][0] = a.n; rem_ws[q][1] = a.flen; rem_ws[q][2] = a.llen; rem_ws[q][3] = a.inside;
        rem_wb[q] = a.fb | (a.lb << 8);
    }
    static __device__ __forceinline__ int finish(u64 &size)
    {
        Agg t = identity();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const Agg o = {rem_ws[q][0], rem_ws[q][1], rem_ws[q][2], rem_ws[q][3], rem_wb[q] & 0xFFu, rem_wb[q] >> 8};
            t = then(t, o);
        }
        size = rem_size<u64>(t);
        return 0;
    }
};

__global__ __launch_bounds__(TP_THREADS) void rle_esize_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                               int nblk, const u64 *__restrict__ d_in_n,
                                                               const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                                               int *__restrict__ err)
{
    tp_blocks<RemBlockSum>(in_cap, tbase, nblk, d_in_n, rec, d_out_n, err);
}

}  // namespace

int rleesize_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                        const u64 *d_in_n, u64 *d_out_n)
{
    return tp_launch(rle_esize_tiles, rle_esize_blocks, bt, st, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_out_n);
}
