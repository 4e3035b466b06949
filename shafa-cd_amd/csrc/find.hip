// find.hip — the positions of a byte pattern in byte regions in device memory (shafa_hipd_find_dev).
//
// A region is block b's d_in_n[b] bytes at d_in + in_off[b], at ANY byte alignment, and no copy of it is made: a lane reads
// the aligned 16-byte words around the 32 bytes it wants and shifts them into place (shift_words, as crc32.hip does).  Such
// a word is only read when it holds at least one byte of the region; every other read is of single bytes inside it.
//
// A match of the m pattern bytes that starts at offset o of region b lies either wholly inside the region (o + m <= n) or in
// its last m - 1 bytes and runs into the regions that follow it in its chain (SHAFA_FIND_NEXT).  The first kind is the tiles'
// work, the second the blocks kernel's, which sees at most 2 (m - 1) bytes; both are charged to region b and the second kind
// has the larger offsets.  Four launches in tile_pass.hpp's shape, no workgroup waits for another, no atomics, the result does
// not depend on scheduling:
//   find_tiles    every 8 KiB tile -> how many matches of the first kind start in each of its four waves (16 bits a wave, the
//                 second word of the tile's 16-byte record).  A lane owns 32 start positions: its eight words and the next
//                 lane's first (a shuffle; the wave's last lane reads four bytes), a filter on the first min(m, 4) bytes — one
//                 v_alignbyte, XOR, AND and compare a position — and the full compare, byte by byte out of the cache, on the
//                 filter's candidates only.  The four waves never meet after the prologue: no barrier in the tile loop.
//   find_blocks   one workgroup per block: an exclusive scan of the block's tile counts (the first word of each record), the
//                 matches of the second kind as a 256-bit mask (bit i: the start i bytes into the block's last min(n, m - 1)),
//                 and d_count[b].
//   find_order    one workgroup: an exclusive scan of d_count over the blocks, from *d_total, which it then advances.
//   find_emit     (max_hits > 0) the tiles whose count is not 0 find their matches again and store them at block base + tile
//                 prefix + wave prefix + lane prefix; then the blocks' masks are stored behind their tiles' matches.  A tile
//                 without a match is not read again.
// Algorithmic HBM bytes: the regions once, 16 bytes per tile written and read twice; a tile with a match twice.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr u32 FIND_MAX = SHAFA_FIND_MAX_PATTERN;
static_assert(FIND_MAX <= TP_THREADS, "a thread per start of the block's last pattern - 1 bytes");
static_assert(TP_THREADS / 64 == 4 && 64 * TP_BPL < 65536, "a record holds four 16-bit wave counts");

__device__ __forceinline__ u32 find_count4(u64 c)
{
    return (u32)(c & 0xFFFF) + (u32)((c >> 16) & 0xFFFF) + (u32)((c >> 32) & 0xFFFF) + (u32)(c >> 48);
}

// The matches that start in this lane's 32 bytes of the tile at pos0 of a region of n bytes at src (src mod 16 = 4 Q + r) and
// lie wholly inside the region: bit j = one starts at pos0 + 32 tid + j.  The aligned word at s16 holds byte p of the region;
// the next two are read where they start in front of the region's end (the third is wanted only when src is not 16-aligned).
// Bytes behind n may sit in the words; no start whose pattern would reach them is looked at.  Every lane of the wave calls.
template <int Q>
__device__ __forceinline__ u32 find_lane(const u8 *src, u64 n, u64 pos0, u32 r, u32 m, u32 pat4, const u8 *pat)
{
    const u32 sh = 4u * Q + r;
    const u64 p = pos0 + (u64)threadIdx.x * TP_BPL;
    u32 w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = 0;
    if (p < n) {
        const u8 *s16 = (const u8 *)(((u64)(uintptr_t)src + p) & ~(u64)15);
        const uint4 zero = make_uint4(0, 0, 0, 0);
        const uint4 a = gload_nt<uint4>(s16);
        uint4 b = zero, c = zero;
        if (p + 16 - sh < n) b = gload_nt<uint4>(s16 + 16);
        if (sh != 0 && p + 32 - sh < n) c = gload_nt<uint4>(s16 + 32);
        const uint4 v0 = sh == 0 ? a : shift_words<Q>(a, b, r), v1 = sh == 0 ? b : shift_words<Q>(b, c, r);
        w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
    }
    // the four bytes behind the lane's: the next lane's first word; the wave's last lane reads them (the halo, at most m - 1
    // bytes into the next wave's or the next tile's part of the same region)
    u32 nx = (u32)__shfl_down((int)w[0], 1, 64);
    if (lane_id() == 63) {
        nx = 0;
#pragma unroll
        for (u32 i = 0; i < 4; ++i)
            if (p + TP_BPL + i < n) nx |= (u32)src[p + TP_BPL + i] << (8 * i);
    }
    w[8] = nx;
    // starts o with o + m <= n
    const u64 starts = n >= m ? n - m + 1 : 0;
    if (p >= starts) return 0;
    const u64 mine = starts - p;
    const u32 valid = mine >= TP_BPL ? 0xFFFFFFFFu : (1u << (u32)mine) - 1u;
    const u32 fmask = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1u;
    u32 cand = 0;
#pragma unroll
    for (int j = 0; j < TP_BPL; ++j) {
        const u32 win = (j & 3) ? __builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], (u32)(j & 3)) : w[j >> 2];
        if (((win ^ pat4) & fmask) == 0) cand |= 1u << j;
    }
    cand &= valid;
    if (m <= 4) return cand;
    u32 hit = 0;
    while (cand) {                                   // the filter's candidates: bytes 4 .. m - 1, all inside the region
        const u32 j = (u32)__builtin_ctz(cand);
        cand &= cand - 1;
        const u8 *q = src + p + j;
        u32 i = 4;
        while (i < m && q[i] == pat[i]) ++i;
        if (i == m) hit |= 1u << j;
    }
    return hit;
}

__device__ __forceinline__ u32 find_lane_any(const u8 *src, u64 n, u64 pos0, u32 m, u32 pat4, const u8 *pat)
{
    const u32 sh = (u32)((uintptr_t)src & 15u), r = sh & 3u;
    switch (sh >> 2) {                               // uniform
    case 0: return find_lane<0>(src, n, pos0, r, m, pat4, pat);
    case 1: return find_lane<1>(src, n, pos0, r, m, pat4, pat);
    case 2: return find_lane<2>(src, n, pos0, r, m, pat4, pat);
    default: return find_lane<3>(src, n, pos0, r, m, pat4, pat);
    }
}

// rec: two 64-bit words a tile: [0] the matches in the block's tiles in front of it (find_blocks), [1] the four wave counts
__global__ __launch_bounds__(TP_THREADS) void find_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                         const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                                         const u64 *__restrict__ d_in_n, const u8 *__restrict__ flags,
                                                         const u8 *__restrict__ d_pat, u32 m, u32 pat4, u64 *__restrict__ rec,
                                                         u32 n_tiles, u32 per_wg)
{
    __shared__ u8 pat[FIND_MAX];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    pat[tid] = d_pat[tid];
    lds_barrier();
    int cur = -1;                                    // the block whose flag is loaded (uniform)
    bool context = false;
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur) {
            cur = wk.b;
            context = (flags[cur] & SHAFA_FIND_CONTEXT) != 0;
        }
        if (context) continue;                       // (uniform) its matches are not reported: find_blocks reads no record
        const u32 hit = find_lane_any(wk.in, wk.n, wk.pos0, m, pat4, pat);
        const u32 c = wave_reduce_add<u32>((u32)__builtin_popcount(hit));
        if (lane == 0) gstore<u16>((u16 *)(rec + 2ull * wk.t + 1) + wv, (u16)c);
    }
}

// seam: four 64-bit words a block, bit i of the 256: a match starts i bytes into the block's last min(n, m - 1) bytes
__global__ __launch_bounds__(TP_THREADS) void find_blocks(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                          const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                                          const u64 *__restrict__ d_in_n, const u8 *__restrict__ flags,
                                                          const u8 *__restrict__ d_pat, u32 m, u64 *__restrict__ rec,
                                                          u64 *__restrict__ seam, u64 *__restrict__ d_count, int *__restrict__ err)
{
    __shared__ u8 pat[FIND_MAX];
    __shared__ u8 buf[2 * FIND_MAX];
    __shared__ u64 wsum[TP_THREADS / 64];
    __shared__ u32 wseam[TP_THREADS / 64];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    pat[tid] = d_pat[tid];
    lds_barrier();
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_in_n[b];
        const u32 fl = flags[b];
        if (n > in_cap[b] || n == 0 || (fl & SHAFA_FIND_CONTEXT)) {     // (uniform) nothing is charged to this block
            if (tid == 0) {
                if (n > in_cap[b]) set_error(err + b, SHAFA_OUTSIDE_MODULE);
                d_count[b] = 0;
            }
            if (tid < TP_THREADS / 64) seam[4ull * b + tid] = 0;
            continue;
        }
        // the tiles' counts, in order
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        u64 *r = rec + 2ull * tbase[b];
        const u32 per = (nt + TP_THREADS - 1) / TP_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        u64 s = 0;
        for (u32 j = lo; j < hi; ++j) s += find_count4(gload<u64>(r + 2ull * j + 1));
        const u64 incl = wave_incl_scan_add<u64>(s);
        if (lane == 63) wsum[wv] = incl;
        // the matches that run into the following regions of the chain
        const u32 tl = n < m - 1 ? (u32)n : m - 1;   // this block's bytes they can start in
        u32 got = 0;                                 // the following regions' bytes, at most m - 1
        if (fl & SHAFA_FIND_NEXT) {                  // (uniform) the last region never has the flag: c + 1 < nblk
            const u8 *src = d_in + in_off[b];
            if ((u32)tid < tl) buf[tid] = src[n - tl + tid];
            for (int c = b; (flags[c] & SHAFA_FIND_NEXT) && got < m - 1;) {
                ++c;
                u64 nc = d_in_n[c];
                if (nc > in_cap[c]) nc = 0;          // counts as empty
                const u32 take = nc < m - 1 - got ? (u32)nc : m - 1 - got;
                if ((u32)tid < take) buf[tl + got + tid] = (d_in + in_off[c])[tid];
                got += take;
            }
        }
        lds_barrier();
        bool hit = (u32)tid < tl && (u32)tid + m <= tl + got;
        if (hit) {
            u32 i = 0;
            while (i < m && buf[tid + i] == pat[i]) ++i;
            hit = i == m;
        }
        const u64 sm = __ballot(hit);
        if (lane == 0) {
            seam[4ull * b + wv] = sm;
            wseam[wv] = (u32)__builtin_popcountll(sm);
        }
        u64 run = incl - s;
#pragma unroll
        for (int q = 0; q < TP_THREADS / 64; ++q)
            if (q < wv) run += wsum[q];
        for (u32 j = lo; j < hi; ++j) {
            gstore<u64>(r + 2ull * j, run);
            run += find_count4(gload<u64>(r + 2ull * j + 1));
        }
        lds_barrier();
        if (tid == 0) {
            u64 total = 0;
#pragma unroll
            for (int q = 0; q < TP_THREADS / 64; ++q) total += wsum[q] + wseam[q];
            d_count[b] = total;
        }
        lds_barrier();                              // the next block of this workgroup writes the wave results and buf
    }
}

// blk_base[b] = *d_total + the counts of the blocks in front of b; *d_total += all counts.  One workgroup.
__global__ __launch_bounds__(TP_THREADS) void find_order(const u64 *__restrict__ d_count, int nblk, u64 *__restrict__ blk_base,
                                                         u64 *d_total)
{
    __shared__ u64 wsum[TP_THREADS / 64];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    u64 carry = gload<u64>(d_total);
    for (int b0 = 0; b0 < nblk; b0 += TP_THREADS) {
        const int b = b0 + tid;
        const u64 v = b < nblk ? d_count[b] : 0ull;
        const u64 incl = wave_incl_scan_add<u64>(v);
        if (lane == 63) wsum[wv] = incl;
        lds_barrier();
        u64 excl = carry + incl - v, total = 0;
#pragma unroll
        for (int q = 0; q < TP_THREADS / 64; ++q) {
            if (q < wv) excl += wsum[q];
            total += wsum[q];
        }
        if (b < nblk) blk_base[b] = excl;
        carry += total;
        lds_barrier();                              // the next round writes the wave sums
    }
    if (tid == 0) gstore<u64>(d_total, carry);       // every thread read it in front of the first barrier
}

__global__ __launch_bounds__(TP_THREADS) void find_emit(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                        const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                                        const u64 *__restrict__ d_in_n, const u8 *__restrict__ flags,
                                                        const u64 *__restrict__ pos, const u8 *__restrict__ d_pat, u32 m, u32 pat4,
                                                        const u64 *__restrict__ rec, const u64 *__restrict__ seam,
                                                        const u64 *__restrict__ blk_base, const u64 *__restrict__ d_count,
                                                        u64 max_hits, u64 *__restrict__ d_hits, u32 n_tiles, u32 per_wg)
{
    __shared__ u8 pat[FIND_MAX];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    pat[tid] = d_pat[tid];
    lds_barrier();
    int cur = -1;                                    // the block whose flag, base and position are loaded (uniform)
    bool context = false;
    u64 base = 0, at = 0;
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur) {
            cur = wk.b;
            context = (flags[cur] & SHAFA_FIND_CONTEXT) != 0;
            base = blk_base[cur];
            at = pos[cur];
        }
        if (context) continue;                       // (uniform) no record
        const u64 cw = gload<u64>(rec + 2ull * wk.t + 1);
        if (cw == 0) continue;                       // (uniform) a tile without a match is not read again
        if (((cw >> (16 * wv)) & 0xFFFF) == 0) continue;                 // (wave uniform; no barrier below)
        u64 k = base + gload<u64>(rec + 2ull * wk.t);
        for (int q = 0; q < wv; ++q) k += (cw >> (16 * q)) & 0xFFFF;
        if (k >= max_hits) continue;                 // (wave uniform)
        u32 hit = find_lane_any(wk.in, wk.n, wk.pos0, m, pat4, pat);
        const u32 c = (u32)__builtin_popcount(hit);
        k += wave_incl_scan_add<u32>(c) - c;
        const u64 p = at + wk.pos0 + (u64)tid * TP_BPL;
        for (; hit && k < max_hits; ++k) {           // ascending
            gstore<u64>(d_hits + k, p + (u32)__builtin_ctz(hit));
            hit &= hit - 1;
        }
    }
    // behind a block's tiles: the matches that run into the following regions
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        u64 k = 0, mine = 0;
        u32 all = 0;
#pragma unroll
        for (int q = 0; q < TP_THREADS / 64; ++q) {
            const u64 s = seam[4ull * b + q];
            const u32 c = (u32)__builtin_popcountll(s);
            if (q < wv) k += c;
            if (q == wv) mine = s;
            all += c;
        }
        if (all == 0) continue;                      // (uniform) also: a block past its region, an empty or a context one
        k += blk_base[b] + d_count[b] - all + (u32)__builtin_popcountll(mine & ((1ull << lane) - 1ull));
        const u64 n = d_in_n[b];
        const u32 tl = n < m - 1 ? (u32)n : m - 1;
        if (((mine >> lane) & 1ull) && k < max_hits) gstore<u64>(d_hits + k, pos[b] + (n - tl) + (u32)tid);
    }
}

}  // namespace

// workspace: tile_setup's with three extras — the positions, the flags (a byte a block) and the pattern, zero padded to
// FIND_MAX; scratch: [records: 16 B per tile of the capacities][block bases: 8 B a block][seam masks: 32 B a block].  The caller
// has checked the arguments.
int find_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                    const u64 *d_in_n, const u8 *h_flags, const u64 *h_pos, const u8 *h_pat, u32 pat_n, u64 max_hits, u64 *d_hits,
                    u64 *d_count, u64 *d_total)
{
    const size_t nb = (size_t)nblocks;
    u8 pat[FIND_MAX] = {};
    memcpy(pat, h_pat, pat_n);
    u32 pat4 = 0;
    for (u32 i = 0; i < 4 && i < pat_n; ++i) pat4 |= (u32)h_pat[i] << (8 * i);
    const TileExtra x[3] = {{h_pos, nb * 8}, {h_flags, nb}, {pat, FIND_MAX}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_in_off, h_in_cap, TP_TILE, x, 3, 16, nb * 40, &a)) return rc;
    const u64 *d_pos = (const u64 *)a.extra[0];
    const u8 *d_flags = a.extra[1], *d_pat = a.extra[2];
    u64 *rec = (u64 *)a.scratch, *blk_base = rec + 2 * (size_t)a.nt, *seam = blk_base + nb;
    if (a.nt)
        hipLaunchKernelGGL(find_tiles, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_in, a.off, a.cap, a.tbase, nblocks, d_in_n, d_flags,
                           d_pat, pat_n, pat4, rec, a.nt, a.per_wg);
    const u32 bw = (u32)nblocks < TP_MAX_BLOCK_WGS ? (u32)nblocks : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(find_blocks, dim3(bw), dim3(TP_THREADS), 0, st, d_in, a.off, a.cap, a.tbase, nblocks, d_in_n, d_flags,
                       d_pat, pat_n, rec, seam, d_count, bt->d_err);
    hipLaunchKernelGGL(find_order, dim3(1), dim3(TP_THREADS), 0, st, (const u64 *)d_count, nblocks, blk_base, d_total);
    if (max_hits && a.nt)                            // a match needs a byte, a byte a tile
        hipLaunchKernelGGL(find_emit, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_in, a.off, a.cap, a.tbase, nblocks, d_in_n, d_flags,
                           d_pos, d_pat, pat_n, pat4, (const u64 *)rec, (const u64 *)seam, (const u64 *)blk_base,
                           (const u64 *)d_count, max_hits, d_hits, a.nt, a.per_wg);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
