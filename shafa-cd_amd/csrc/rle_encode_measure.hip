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
// The tiles of all blocks are numbered consecutively (from the capacities, on the host) and dealt to the workgroups in equal
// runs, so the grid is the call's tile count whatever the mix of block sizes.
//
// Algorithmic HBM bytes per block: n read, 16 bytes per 8 KiB tile written and read again.
#include "common.hpp"
#include "internal.hpp"

namespace {

constexpr int RES_THREADS = 256;
constexpr int RES_BPL = 32;                        // bytes per lane
constexpr int RES_TILE = RES_THREADS * RES_BPL;
constexpr u32 RES_MAX_WGS = 16384;                 // rle_esize_tiles: workgroups per launch
constexpr u32 RES_MAX_BLOCK_WGS = 1u << 20;        // rle_esize_blocks: workgroups per launch (grid-stride over the blocks)

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

// the piece held by lanes [l, l + 2 d) after the step of distance d: an ordered reduction, lane 0 ends with the wave's
template <typename T>
__device__ __forceinline__ Rem<T> rem_wave_reduce(Rem<T> a)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Rem<T> o;
        o.n = (T)__shfl_down(a.n, d, 64);
        o.flen = (T)__shfl_down(a.flen, d, 64);
        o.llen = (T)__shfl_down(a.llen, d, 64);
        o.inside = (T)__shfl_down(a.inside, d, 64);
        const u32 e = (u32)__shfl_down((int)(a.fb | (a.lb << 8)), d, 64);
        o.fb = e & 0xFFu;
        o.lb = e >> 8;
        if (lane + d < 64) a = rem_then<T>(a, o);
    }
    return a;
}

// the block of global tile t: the largest b with tbase[b] <= t (tbase is non-decreasing, tbase[0] = 0, tbase[nblk] > t);
// a 64-way search, every lane of the wave returns the same b
__device__ __forceinline__ int res_find_block(const u32 *__restrict__ tbase, int nblk, u32 t)
{
    const int lane = lane_id();
    int lo = 0, hi = nblk;
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

// a run shorter than 255 bytes
__device__ __forceinline__ u32 res_short_cost(u32 s, u32 L) { return s == 0 ? 3u : (L < 3u ? L : 3u); }

__global__ __launch_bounds__(RES_THREADS) void rle_esize_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                               const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                               int nblk, const u64 *__restrict__ d_in_n,
                                                               uint4 *__restrict__ rec, u32 n_tiles, u32 per_wg)
{
    __shared__ __attribute__((aligned(16))) uint4 sh_a[2][4];      // per tile parity and wave: {n | flen << 16, llen | fb << 16 | lb << 24, inside, -}
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const u64 first = (u64)blockIdx.x * per_wg;
    if (first >= n_tiles) return;
    const u32 t_end = first + per_wg < n_tiles ? (u32)(first + per_wg) : n_tiles;
    int b = res_find_block(tbase, nblk, (u32)first);
    u32 tb = tbase[b], tnext = tbase[b + 1];
    bool fresh = true;
    u64 n = 0;
    const u8 *in = d_in;
    u32 turn = 0;
    for (u32 t = (u32)first; t < t_end; ++t) {
        while (t >= tnext) {                        // (uniform) tbase[nblk] = n_tiles > t ends it
            ++b;
            tb = tnext;
            tnext = tbase[b + 1];
            fresh = true;
        }
        if (fresh) {
            n = d_in_n[b];
            if (n > in_cap[b]) n = 0;               // SHAFA_OUTSIDE_MODULE, reported by rle_esize_blocks: no byte of it is read
            in = d_in + in_off[b];
            fresh = false;
        }
        const u64 pos0 = (u64)(t - tb) * RES_TILE;
        if (pos0 >= n) continue;                    // (uniform) past the block's real size: no record is read there

        // ---- the lane's 32 bytes; bytes past the block's end are never loaded ---------------------------------------------
        const u64 pos = pos0 + (u64)tid * RES_BPL;
        u32 w[8];
        u32 nvalid;
        if (pos + RES_BPL <= n) {
            const uint4 v0 = gload_nt<uint4>(in + pos), v1 = gload_nt<uint4>(in + pos + 16);
            w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
            nvalid = RES_BPL;
        } else {
            nvalid = pos < n ? (u32)(n - pos) : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = 0;
#pragma unroll
            for (int j = 0; j < RES_BPL; ++j)
                if ((u32)j < nvalid) w[j >> 2] |= (u32)in[pos + j] << (8 * (j & 3));
        }
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
        if (__all(!one && nvalid == (u32)RES_BPL)) {
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
            a.n = 64u * RES_BPL;                    // lane 0 keeps its own first byte and first run
        } else {
            a = rem_wave_reduce<u32>(a);
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
            gstore<uint4>(rec + t, make_uint4(r.n | (r.fb << 16) | (r.lb << 24), r.flen, r.llen, r.inside));
        }
        // the next tile writes the other set of slots; this set is written again after the next tile's barrier, which
        // thread 0 reaches only after it has read these
    }
}

__global__ __launch_bounds__(RES_THREADS) void rle_esize_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                                int nblk, const u64 *__restrict__ d_in_n,
                                                                const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                                                int *__restrict__ err)
{
    __shared__ u64 ws[4][4];
    __shared__ u32 wb[4];
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
        const u32 nt = (u32)((n + RES_TILE - 1) / RES_TILE);
        const uint4 *r = rec + tbase[b];
        const u32 per = (nt + RES_THREADS - 1) / RES_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        Rem<u64> a = {0, 0, 0, 0, 0, 0};
        for (u32 j = lo; j < hi; ++j) {
            const uint4 v = gload<uint4>(r + j);
            const Rem<u64> o = {v.x & 0xFFFFu, v.y, v.z, v.w, (v.x >> 16) & 0xFFu, v.x >> 24};
            a = rem_then<u64>(a, o);
        }
        a = rem_wave_reduce<u64>(a);
        if (lane == 0) {
            ws[wv][0] = a.n; ws[wv][1] = a.flen; ws[wv][2] = a.llen; ws[wv][3] = a.inside;
            wb[wv] = a.fb | (a.lb << 8);
        }
        lds_barrier();
        if (tid == 0) {
            Rem<u64> t = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const Rem<u64> o = {ws[q][0], ws[q][1], ws[q][2], ws[q][3], wb[q] & 0xFFu, wb[q] >> 8};
                t = rem_then<u64>(t, o);
            }
            d_out_n[b] = rem_size<u64>(t);
        }
        lds_barrier();                              // the next block of this workgroup writes ws / wb
    }
}

}  // namespace

int rleesize_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                        const u64 *d_in_n, u64 *d_out_n)
{
    u64 ntiles = 0;
    for (int b = 0; b < nblocks; ++b) ntiles += ceil_div_u64(h_in_cap[b], RES_TILE);
    if (ntiles > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    // workspace: the tile records, then what the host uploads: offsets, capacities, first tile numbers
    const size_t nb = (size_t)nblocks;
    const size_t o_rec = 0, o_up = (size_t)ntiles * 16;
    const size_t u_off = 0, u_cap = nb * 8, u_base = 2 * nb * 8, up_bytes = (2 * nb * 8 + (nb + 1) * 4 + 15) & ~(size_t)15;
    int rc = batch_reserve(bt, st, o_up + up_bytes);
    if (rc) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    u8 *hs = (u8 *)batch_stage(bt, st, up_bytes);
    if (!hs) return SHAFA_LACK_OF_MEMORY;
    memcpy(hs + u_off, h_in_off, nb * 8);
    memcpy(hs + u_cap, h_in_cap, nb * 8);
    u32 *hb = (u32 *)(hs + u_base);
    u32 base = 0;
    for (int b = 0; b < nblocks; ++b) {
        hb[b] = base;
        base += (u32)ceil_div_u64(h_in_cap[b], RES_TILE);
    }
    hb[nblocks] = base;
    memset(hs + u_base + (nb + 1) * 4, 0, up_bytes - (u_base + (nb + 1) * 4));
    if ((rc = batch_upload(bt, st, ws + o_up, hs, up_bytes))) return rc;
    const u64 *d_off = (const u64 *)(ws + o_up + u_off), *d_cap = (const u64 *)(ws + o_up + u_cap);
    const u32 *d_base = (const u32 *)(ws + o_up + u_base);
    if (ntiles) {
        const u32 nt = (u32)ntiles, per_wg = (nt + RES_MAX_WGS - 1) / RES_MAX_WGS, wgs = (nt + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(rle_esize_tiles, dim3(wgs), dim3(RES_THREADS), 0, st, d_in, d_off, d_cap, d_base, nblocks, d_in_n,
                           (uint4 *)(ws + o_rec), nt, per_wg);
    }
    const u32 bw = (u32)nblocks < RES_MAX_BLOCK_WGS ? (u32)nblocks : RES_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(rle_esize_blocks, dim3(bw), dim3(RES_THREADS), 0, st, d_cap, d_base, nblocks, d_in_n,
                       (const uint4 *)(ws + o_rec), d_out_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
