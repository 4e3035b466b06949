// tile_pass.hpp — the skeleton of a size pass: what rle_measure.hip (decoded sizes) and rle_encode_measure.hip (encoded sizes)
// share.  A pass summarises every 8 KiB tile of every block in a 16-byte record (its tiles kernel), then puts each block's
// records together in order (its blocks kernel); the two passes differ only in the summary.  Here:
//   geometry        TP_*: 256 lanes x 32 bytes a tile, the workgroup bounds of the two launches
//   TpWalk          the tiles kernel's loop: the workgroup's run of global tile numbers, the block each tile lies in, the two
//                   uniform skips; the pass writes the body of one tile.  (A cursor, not a function taking the body: handed
//                   over as a lambda, however captured and inlined, rle_measure_tiles' body cost one more VGPR.)
//   tp_lane_load    the lane's 32 bytes of a tile
//   tp_wave_reduce  an ordered reduction of summaries across the wave
//   tp_blocks       the blocks kernel's body over a summary trait
//   tp_launch       the host launcher: both launches, on the workspace that tile_setup (internal.hpp) lays out and uploads
// The tiles of all blocks are numbered consecutively (from the capacities, on the host: tile_setup) and dealt to the workgroups
// in equal runs, so the grid is the call's tile count (at most TP_MAX_WGS workgroups) whatever the mix of block sizes.
#pragma once

#include "common.hpp"
#include "internal.hpp"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_BPL = 32;                         // bytes per lane
constexpr int TP_TILE = TP_THREADS * TP_BPL;
// (TP_MAX_WGS, the tiles kernel's workgroups per launch, is internal.hpp's: tile_setup deals the tiles out)
constexpr u32 TP_MAX_BLOCK_WGS = 1u << 20;         // blocks kernel: workgroups per launch (grid-stride over the blocks)

// the block of global tile t: the largest b with tbase[b] <= t (tbase is non-decreasing, tbase[0] = 0, tbase[nblk] > t);
// a 64-way search, every lane of the wave returns the same b
__device__ __forceinline__ int tp_find_block(const u32 *__restrict__ tbase, int nblk, u32 t)
{
    const int lane = lane_id();
    int lo = 0, hi = nblk;                          // tbase[lo] <= t, answer in [lo, hi)
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) / 64;
        const int idx = lo + lane * step;
        const bool le = idx < hi && tbase[idx] <= t;
        const int p = __builtin_popcountll(__ballot(le)) - 1;      // lane 0 always holds (idx = lo)
        lo += p * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// The workgroup's tiles [blockIdx.x * per_wg, + per_wg) in order, and the block each lies in:
//     for (TpWalk wk(...); wk.more(); wk.step()) { if (!wk.enter()) continue; ... one tile ... }
// After enter() global tile t is tile k of a block whose input is at `in` and has n real bytes, pos0 = k * TP_TILE < n.  All
// members are uniform.
struct TpWalk {
    const u8 *d_in;
    const u64 *in_off, *in_cap;
    const u32 *tbase;
    const u64 *d_in_n;
    u32 t, t_end, k;
    int b;
    u32 tb, tnext;
    bool fresh;
    u64 n, pos0;
    const u8 *in;
    __device__ __forceinline__ TpWalk(const u8 *__restrict__ d_in_, const u64 *__restrict__ in_off_, const u64 *__restrict__ in_cap_,
                                      const u32 *__restrict__ tbase_, int nblk, const u64 *__restrict__ d_in_n_, u32 n_tiles,
                                      u32 per_wg)
        : d_in(d_in_), in_off(in_off_), in_cap(in_cap_), tbase(tbase_), d_in_n(d_in_n_), t(0), t_end(0), k(0), b(0), tb(0),
          tnext(0), fresh(true), n(0), pos0(0), in(d_in_)
    {
        const u64 first = (u64)blockIdx.x * per_wg;
        if (first >= n_tiles) return;               // no tile: more() is false
        t = (u32)first;
        t_end = first + per_wg < n_tiles ? (u32)(first + per_wg) : n_tiles;
        b = tp_find_block(tbase, nblk, t);
        tb = tbase[b];
        tnext = tbase[b + 1];
    }
    __device__ __forceinline__ bool more() const { return t < t_end; }
    __device__ __forceinline__ void step() { ++t; }
    // false: the tile lies past its block's real size (no record is read there)
    __device__ __forceinline__ bool enter()
    {
        while (t >= tnext) {                        // (uniform) tbase[nblk] = n_tiles > t ends it
            ++b;
            tb = tnext;
            tnext = tbase[b + 1];
            fresh = true;
        }
        if (fresh) {
            n = d_in_n[b];
            if (n > in_cap[b]) n = 0;               // SHAFA_OUTSIDE_MODULE, reported by the blocks kernel: no byte of it is read
            in = d_in + in_off[b];
            fresh = false;
        }
        k = t - tb;
        pos0 = (u64)k * TP_TILE;
        return pos0 < n;                            // (uniform)
    }
};

// the lane's 32 bytes of the tile at pos0, little-endian in w; returns how many of them lie inside the block (the others
// are 0 and are never loaded)
__device__ __forceinline__ u32 tp_lane_load(const u8 *in, u64 pos0, u64 n, u32 (&w)[8])
{
    const u64 pos = pos0 + (u64)threadIdx.x * TP_BPL;
    if (pos + TP_BPL <= n) {
        const uint4 v0 = gload_nt<uint4>(in + pos), v1 = gload_nt<uint4>(in + pos + 16);
        w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
        return TP_BPL;
    }
    const u32 nvalid = pos < n ? (u32)(n - pos) : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = 0;
#pragma unroll
    for (int j = 0; j < TP_BPL; ++j)
        if ((u32)j < nvalid) w[j >> 2] |= (u32)in[pos + j] << (8 * (j & 3));
    return nvalid;
}

// byte k of a 16-byte word
__device__ __forceinline__ u8 tp_byte_of(const uint4 &v, int k)
{
    const u32 x[4] = {v.x, v.y, v.z, v.w};
    return (u8)(x[k >> 2] >> (8 * (k & 3)));
}

// for a pass without a blocks kernel (planes.hip, records.hip): a block whose size is past its capacity — the walk has skipped
// its tiles (a capacity of 0 has none), this reports it
__device__ __forceinline__ void tp_size_errors(const u64 *__restrict__ cap, const u64 *__restrict__ d_n, int nblk, int *__restrict__ err)
{
    for (u64 b = (u64)blockIdx.x * TP_THREADS + threadIdx.x; b < (u64)nblk; b += (u64)gridDim.x * TP_THREADS)
        if (d_n[b] > cap[b]) set_error(err + b, SHAFA_OUTSIDE_MODULE);
}

// A summary trait S: Agg (the summary of a piece), then(a, b) (associative: a's piece, then b's) and from_lane(a, d) (lane
// l + d's a).  After the step of distance d lane l holds lanes [l, l + 2 d) of the wave: lane 0 ends with the wave's.
template <typename S>
__device__ __forceinline__ typename S::Agg tp_wave_reduce(typename S::Agg a)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const typename S::Agg o = S::from_lane(a, d);
        if (lane + d < 64) a = S::then(a, o);
    }
    return a;
}

// The blocks kernel: one workgroup per block (grid-stride).  Each thread composes a run of consecutive records, an ordered
// reduction puts each wave's together, thread 0 finishes.  Beyond tp_wave_reduce's, S gives identity(), read(record),
// put(q, a) (wave q's result, into LDS of the pass's own) and finish(size): the four wave results in order -> the block's
// size and its error code or 0.  (The compose of the four is the pass's: the decoded sizes follow one entry state through
// them, which a general then() over all three costs 4 VGPRs; and the wave results are arrays of the pass's, one per field
// width, because one LDS struct for both widths changed the address arithmetic and with it rle_esize_blocks' VGPR count.)
template <typename S>
__device__ __forceinline__ void tp_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                          const u64 *__restrict__ d_in_n, const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                          int *__restrict__ err)
{
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_in_n[b];
        if (n > in_cap[b]) {                        // (uniform) past the block's region
            if (tid == 0) {
                set_error(err + b, SHAFA_OUTSIDE_MODULE);
                d_out_n[b] = 0;
            }
            continue;
        }
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        const uint4 *r = rec + tbase[b];
        const u32 per = (nt + TP_THREADS - 1) / TP_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        typename S::Agg a = S::identity();
        for (u32 j = lo; j < hi; ++j) a = S::then(a, S::read(gload<uint4>(r + j)));
        a = tp_wave_reduce<S>(a);
        if (lane == 0) S::put(wv, a);
        lds_barrier();
        if (tid == 0) {
            u64 size;
            const int code = S::finish(size);
            if (code) set_error(err + b, code);
            d_out_n[b] = size;
        }
        lds_barrier();                              // the next block of this workgroup writes the wave results
    }
}

using TpTilesKernel = void (*)(const u8 *, const u64 *, const u64 *, const u32 *, int, const u64 *, uint4 *, u32, u32);
using TpBlocksKernel = void (*)(const u64 *, const u32 *, int, const u64 *, const uint4 *, u64 *, int *);

// workspace: tile_setup's with no extra; scratch: the records, 16 B per tile of the capacities
inline int tp_launch(TpTilesKernel tiles, TpBlocksKernel blocks, Batch *bt, hipStream_t st, int nblocks, const u8 *d_in,
                     const u64 *h_in_off, const u64 *h_in_cap, const u64 *d_in_n, u64 *d_out_n)
{
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_in_off, h_in_cap, TP_TILE, nullptr, 0, 16, 0, &a)) return rc;
    if (a.nt)
        hipLaunchKernelGGL(tiles, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_in, a.off, a.cap, a.tbase, nblocks, d_in_n,
                           (uint4 *)a.scratch, a.nt, a.per_wg);
    const u32 bw = (u32)nblocks < TP_MAX_BLOCK_WGS ? (u32)nblocks : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(blocks, dim3(bw), dim3(TP_THREADS), 0, st, a.cap, a.tbase, nblocks, d_in_n, (const uint4 *)a.scratch,
                       d_out_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

}  // namespace
