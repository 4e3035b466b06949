// compare.hip — where a decoder's output blocks first differ from an original (shafa_hipd_compare_dev).
//
// Side a is what a device decoder leaves: 16-aligned regions whose sizes (d_a_n) live in device memory.  Side ref is the
// original, block b's bytes at d_ref + ref_off[b] at ANY byte alignment, and no copy of it is made: a lane reads the two
// aligned 16-byte words around the 16 bytes it wants and shifts them into place (shift_words, as pack_bulk does for its
// sources).  Such a word is only read when it holds at least one byte of [ref, ref + ref_n) — memory is handed out in units
// far larger than 16 bytes, so the rest of the word is readable — and no byte of ref is read in any other way.
//
// With m = min(a_n, ref_n): first[b] = the smallest i < m with a[i] != ref[i], or m.  Bytes of the region behind a_n (the
// slack of an exact region is uninitialised) and bytes of ref behind ref_n are masked out of every word before it counts.
// A difference is data: no error word is set for it.  a_n > a_cap is SHAFA_OUTSIDE_MODULE, first[b] = 0, nothing is read.
//
// Two launches in tile_pass.hpp's shape, no workgroup waits for another, no atomics, the result does not depend on scheduling:
//   compare_tiles   every 8 KiB tile below m -> one 16-byte record: per wave the smallest offset (within the tile) at which
//                   the wave's 2 x 64 words differ, or CMP_NONE.  The four waves of a workgroup never meet: no LDS, no
//                   barrier.  The walk over the tiles of all blocks is TpWalk.
//   compare_blocks  one workgroup per block: the smallest (tile, offset) of the block's records, which is the first in
//                   block order; thread 0 writes first[b].
// Algorithmic HBM bytes per block: 2 m read (both operands once, non-temporal), 16 bytes per tile written and read again.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr u32 CMP_NONE = 0xFFFFFFFFu;
constexpr int CMP_WORDS = TP_TILE / 16 / TP_THREADS;       // 16-byte words per lane and tile

// the 16 bytes of side a at p (p < m <= a_n): whole where the block has them, else its last bytes one by one
__device__ __forceinline__ uint4 cmp_load_a(const u8 *a, u64 a_n, u64 p)
{
    if (p + 16 <= a_n) return gload_nt<uint4>(a + p);
    const u32 nvalid = (u32)(a_n - p);
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 15; ++j)
        if ((u32)j < nvalid) w[j >> 2] |= (u32)a[p + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// index of the first non-zero byte of x, 16 when there is none
__device__ __forceinline__ u32 cmp_first_byte(const uint4 &x)
{
    u32 i = 16;
    if (x.w) i = 12 + ((u32)__builtin_ctz(x.w) >> 3);
    if (x.z) i = 8 + ((u32)__builtin_ctz(x.z) >> 3);
    if (x.y) i = 4 + ((u32)__builtin_ctz(x.y) >> 3);
    if (x.x) i = (u32)__builtin_ctz(x.x) >> 3;
    return i;
}

// One tile of one wave: bytes [pos0, min(pos0 + TP_TILE, m)) of the block, word k * TP_THREADS + tid to this lane.  ref's
// address is 4 Q + r (mod 16); sh = 4 Q + r.  -> the wave's smallest differing offset within the tile, or CMP_NONE (uniform).
template <int Q>
__device__ __forceinline__ u32 cmp_tile(const u8 *a, u64 a_n, const u8 *ref, u64 ref_n, u64 m, u64 pos0, u32 r)
{
    const u32 sh = 4u * Q + r;
    uint4 va[CMP_WORDS], lo[CMP_WORDS], hi[CMP_WORDS];
#pragma unroll
    for (int k = 0; k < CMP_WORDS; ++k) {
        const u64 p = pos0 + 16ull * (u32)(k * TP_THREADS + (int)threadIdx.x);
        hi[k] = make_uint4(0, 0, 0, 0);
        if (p < m) {
            va[k] = cmp_load_a(a, a_n, p);
            // ref byte p lies in the aligned word at s16, which therefore holds a byte of the range; the next word does if
            // it starts in front of ref + ref_n (its bytes are wanted only when ref is not 16-aligned)
            const u8 *s16 = (const u8 *)(((u64)(uintptr_t)ref + p) & ~(u64)15);
            lo[k] = gload_nt<uint4>(s16);
            if (sh != 0 && p + 16 - sh < ref_n) hi[k] = gload_nt<uint4>(s16 + 16);
        }
    }
    u32 best = CMP_NONE;
#pragma unroll
    for (int k = CMP_WORDS - 1; k >= 0; --k) {
        const u32 wo = 16u * (u32)(k * TP_THREADS + (int)threadIdx.x);
        const u64 p = pos0 + wo;
        if (p < m) {
            const uint4 vr = sh == 0 ? lo[k] : shift_words<Q>(lo[k], hi[k], r);
            const u32 i = cmp_first_byte(make_uint4(va[k].x ^ vr.x, va[k].y ^ vr.y, va[k].z ^ vr.z, va[k].w ^ vr.w));
            const u64 left = m - p;                 // bytes of the word that count: the others are slack, or past ref's end
            if (i < 16 && i < left) best = wo + i;  // word k is in front of word k + 1: the last assignment is the smallest
        }
    }
    // the lowest lane with a difference in word 0 holds the wave's smallest offset, else the lowest lane with one in word 1, ...
    u32 res = CMP_NONE;
#pragma unroll
    for (int k = CMP_WORDS - 1; k >= 0; --k) {
        const u32 lim = 16u * (u32)((k + 1) * TP_THREADS);
        const u64 hit = __ballot(best < lim);
        if (hit) res = (u32)__builtin_amdgcn_readlane((int)best, __builtin_ctzll(hit));
    }
    return res;
}

__global__ __launch_bounds__(TP_THREADS) void compare_tiles(const u8 *__restrict__ d_a, const u64 *__restrict__ a_off,
                                                            const u64 *__restrict__ a_cap, const u32 *__restrict__ tbase, int nblk,
                                                            const u64 *__restrict__ d_a_n, const u8 *__restrict__ d_ref,
                                                            const u64 *__restrict__ ref_off, const u64 *__restrict__ ref_n,
                                                            u32 *__restrict__ rec, u32 n_tiles, u32 per_wg)
{
    const int lane = lane_id(), wv = wave_id();
    int cur = -1;                                   // the block whose ref and m are loaded (uniform)
    const u8 *ref = d_ref;
    u64 rn = 0, m = 0;
    for (TpWalk wk(d_a, a_off, a_cap, tbase, nblk, d_a_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur) {
            cur = wk.b;
            rn = ref_n[cur];
            ref = d_ref + ref_off[cur];
            m = wk.n < rn ? wk.n : rn;
        }
        if (wk.pos0 >= m) continue;                 // (uniform) compare_blocks reads the records of the tiles below m only
        const u32 sh = (u32)((uintptr_t)ref & 15u), r = sh & 3u;
        u32 res;
        switch (sh >> 2) {                          // uniform
        case 0: res = cmp_tile<0>(wk.in, wk.n, ref, rn, m, wk.pos0, r); break;
        case 1: res = cmp_tile<1>(wk.in, wk.n, ref, rn, m, wk.pos0, r); break;
        case 2: res = cmp_tile<2>(wk.in, wk.n, ref, rn, m, wk.pos0, r); break;
        default: res = cmp_tile<3>(wk.in, wk.n, ref, rn, m, wk.pos0, r); break;
        }
        if (lane == 0) gstore<u32>(rec + 4ull * wk.t + (u32)wv, res);
    }
}

__global__ __launch_bounds__(TP_THREADS) void compare_blocks(const u64 *__restrict__ a_cap, const u32 *__restrict__ tbase, int nblk,
                                                             const u64 *__restrict__ d_a_n, const u64 *__restrict__ ref_n,
                                                             const uint4 *__restrict__ rec, u64 *__restrict__ d_first,
                                                             int *__restrict__ err)
{
    __shared__ u64 wfirst[TP_THREADS / 64];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_a_n[b];
        if (n > a_cap[b]) {                         // (uniform) past the block's region
            if (tid == 0) {
                set_error(err + b, SHAFA_OUTSIDE_MODULE);
                d_first[b] = 0;
            }
            continue;
        }
        const u64 rn = ref_n[b], m = n < rn ? n : rn;
        const u32 nt = (u32)((m + TP_TILE - 1) / TP_TILE);
        const uint4 *r = rec + tbase[b];
        u64 first = m;                              // offsets in front of m only: the smallest one, or m
        for (u32 j = (u32)tid; j < nt; j += TP_THREADS) {       // ascending: the thread's first hit is its smallest
            const uint4 v = gload<uint4>(r + j);
            const u32 a01 = v.x < v.y ? v.x : v.y, a23 = v.z < v.w ? v.z : v.w, o = a01 < a23 ? a01 : a23;
            if (o != CMP_NONE) {
                first = (u64)j * TP_TILE + o;
                break;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u64 o = (u64)__shfl_xor((unsigned long long)first, d, 64);
            first = o < first ? o : first;
        }
        if (lane == 0) wfirst[wv] = first;
        lds_barrier();
        if (tid == 0) {
            u64 f = wfirst[0];
#pragma unroll
            for (int q = 1; q < TP_THREADS / 64; ++q) f = wfirst[q] < f ? wfirst[q] : f;
            d_first[b] = f;
        }
        lds_barrier();                              // the next block of this workgroup writes the wave results
    }
}

}  // namespace

// workspace: tile_setup's with two extras, ref_off and ref_n; scratch: the records, 16 B per tile of a's capacities
int compare_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_a, const u64 *h_a_off, const u64 *h_a_cap,
                       const u64 *d_a_n, const u8 *d_ref, const u64 *h_ref_off, const u64 *h_ref_n, u64 *d_first)
{
    const TileExtra x[2] = {{h_ref_off, (size_t)nblocks * 8}, {h_ref_n, (size_t)nblocks * 8}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_a_off, h_a_cap, TP_TILE, x, 2, 16, 0, &a)) return rc;
    const u64 *d_roff = (const u64 *)a.extra[0], *d_rn = (const u64 *)a.extra[1];
    if (a.nt)
        hipLaunchKernelGGL(compare_tiles, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_a, a.off, a.cap, a.tbase, nblocks, d_a_n, d_ref,
                           d_roff, d_rn, (u32 *)a.scratch, a.nt, a.per_wg);
    const u32 bw = (u32)nblocks < TP_MAX_BLOCK_WGS ? (u32)nblocks : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(compare_blocks, dim3(bw), dim3(TP_THREADS), 0, st, a.cap, a.tbase, nblocks, d_a_n, d_rn,
                       (const uint4 *)a.scratch, d_first, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
