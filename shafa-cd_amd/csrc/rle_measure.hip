// rle_measure.hip — the decoded size of RLE blocks without decoding them (shafa_hipd_rle_decoded_size_dev).
//
// The decoder (rle_decode.hip) learns a block's size by writing its output; this is the same token machine (rld_fsm.hpp)
// with a sum in place of the output image.  A run is charged to its COUNT byte: a byte met in state S2 adds `count ? count
// : 1` (d.c:179-184), a non-zero byte met in S0 adds 1, everything else adds 0.  So what a piece of the stream adds depends
// on its own bytes and on the state it is entered in, and on nothing else — a triple that straddles two pieces needs no
// special case — and (map, sum per entry state) composes in order like the maps alone:
//     (A then B).map = fn_compose(A.map, B.map)      (A then B).sum[s] = A.sum[s] + B.sum[A.map(s)]
// Two launches, no workgroup ever waits for another (no tickets, no descriptors, no agent-scope atomics):
//   rle_measure_tiles   every 8 KiB tile -> one 16-byte record {map, sum[S0], sum[S1], sum[S2]} (sums < 85 x 8 KiB: 32 bits).
//                       The 32 bytes in front of a tile nearly always settle the state whatever it was before them (two
//                       non-zero bytes in a row end in S0): then the tile is entered in a known state, each lane adds up
//                       once, and the record is written as a constant map with three equal sums.  Only a tile behind 32
//                       zero-heavy bytes adds up three times.
//   rle_measure_blocks  one workgroup per block: each thread composes a run of consecutive records, an ordered
//                       reduction lanes -> waves -> block puts them together, thread 0 checks the exit state (not S0: the
//                       stream ends inside a triple) and SHAFA_RLE_DECODE_MAX and writes d_out_n[b] and the error word.
// The tiles of all blocks are numbered consecutively (from the capacities, on the host) and dealt to the workgroups in
// equal runs; a workgroup finds the block of its first tile by a 64-way search over the blocks' first tile numbers and
// walks on from there.  The grid is therefore the number of tiles (at most RLM_MAX_WGS workgroups), whatever the mix of
// block sizes: one 64 MiB block next to thousands of small ones costs its own tiles and theirs, not their product.
//
// Algorithmic HBM bytes per block: rle_n read, 16 bytes per 8 KiB tile written and read again.
#include "common.hpp"
#include "internal.hpp"
#include "rld_fsm.hpp"

namespace {

constexpr u32 RLM_MAX_WGS = 16384;                 // rle_measure_tiles: workgroups per launch (64 a CU, 8 of them resident at a time)
constexpr u32 RLM_MAX_BLOCK_WGS = 1u << 20;        // rle_measure_blocks: workgroups per launch (grid-stride over the blocks)

struct RlmShared {
    u32 fsm[256];
    u32 wfn[4];
    u32 wsum[3][4];
};

// the block of global tile t: the largest b with tbase[b] <= t (tbase is non-decreasing, tbase[0] = 0, tbase[nblk] > t);
// every lane of the wave returns the same b
__device__ __forceinline__ int rlm_find_block(const u32 *__restrict__ tbase, int nblk, u32 t)
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

// what the lane's valid bytes add when the lane is entered in state es
__device__ __forceinline__ u32 rlm_lane_sum(const u32 (&st3)[3], const u32 (&wp)[8], u32 z, u32 vm, u32 es)
{
    const u32 S = (es == 0 ? st3[0] : es == 1 ? st3[1] : st3[2]) & vm;
    const u32 E = S & z;                                            // escapes: their count bytes sit two places on
    const u32 Cm = ((E << 2) | (es == 2 ? 1u : es == 1 ? 2u : 0u)) & vm;
    u32 acc = (u32)__builtin_popcount(S & ~z);                      // literals
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_udot4(wp[i], nib_flags(Cm, i), acc, false);
    return acc;
}

__global__ __launch_bounds__(RLD_THREADS) void rle_measure_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                                 const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                                 int nblk, const u64 *__restrict__ d_in_n,
                                                                 uint4 *__restrict__ rec, u32 n_tiles, u32 per_wg)
{
    __shared__ __attribute__((aligned(16))) RlmShared sh;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const u64 first = (u64)blockIdx.x * per_wg;
    if (first >= n_tiles) return;
    const u32 t_end = first + per_wg < n_tiles ? (u32)(first + per_wg) : n_tiles;
    sh.fsm[tid] = g_rld_fsm.v[tid];
    lds_barrier();
    int b = rlm_find_block(tbase, nblk, (u32)first);
    u32 tb = tbase[b], tnext = tbase[b + 1];
    bool fresh = true;
    u64 n = 0;
    const u8 *in = d_in;
    for (u32 t = (u32)first; t < t_end; ++t) {
        while (t >= tnext) {                        // (uniform) tbase[nblk] = n_tiles > t ends it
            ++b;
            tb = tnext;
            tnext = tbase[b + 1];
            fresh = true;
        }
        if (fresh) {
            n = d_in_n[b];
            if (n > in_cap[b]) n = 0;               // SHAFA_OUTSIDE_MODULE, reported by rle_measure_blocks: no byte of it is read
            in = d_in + in_off[b];
            fresh = false;
        }
        const u32 k = t - tb;
        const u64 pos0 = (u64)k * RLD_TILE;
        if (pos0 >= n) continue;                    // (uniform) past the block's real size: no record is read there

        // ---- the lane's 32 bytes, their zero mask, and the bytes with 0 replaced by 1 (a count of 0 acts as 1) ----------
        const u64 pos = pos0 + (u64)tid * RLD_BPL;
        u32 w[8];
        int nvalid;
        if (pos + RLD_BPL <= n) {
            const uint4 v0 = gload_nt<uint4>(in + pos), v1 = gload_nt<uint4>(in + pos + 16);
            w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
            nvalid = RLD_BPL;
        } else {
            nvalid = pos < n ? (int)(n - pos) : 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = 0;
#pragma unroll
            for (int j = 0; j < RLD_BPL; ++j)
                if (j < nvalid) w[j >> 2] |= (u32)in[pos + j] << (8 * (j & 3));
        }
        // the map of the 32 bytes in front of the tile (one address for all lanes): constant nearly always, and then its
        // value IS the state the tile is entered in.  Tile 0 is entered in S0.
        u32 fprev = 0;
        if (k > 0) {
            const uint4 p0 = gload<uint4>(in + pos0 - 32), p1 = gload<uint4>(in + pos0 - 16);
            const u32 pw[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            u32 pst[3], pex[3];
            fsm32(sh.fsm, zmask32(pw), pst, pex);
            fprev = pex[0] | (pex[1] << 2) | (pex[2] << 4);
        }
        const u32 vm = nvalid >= 32 ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
        const u32 z = zmask32(w) & vm;
        u32 wp[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wp[i] = w[i] | (zero_bytes80(w[i]) >> 7);

        // ---- the lane's map; bytes past the end of the block do not move the state ---------------------------------------
        u32 st3[3], ex3[3];
        if (__all(z == 0u && nvalid == RLD_BPL)) {  // a wave without a zero byte: literals once the state is S0
            st3[0] = 0xFFFFFFFFu; st3[1] = 0xFFFFFFFCu; st3[2] = 0xFFFFFFFEu;
            ex3[0] = ex3[1] = ex3[2] = 0;
        } else {
            fsm32(sh.fsm, z, st3, ex3);
            if (nvalid < RLD_BPL) {                 // the table ran over 32 bytes: walk the valid ones (the block's last lane)
#pragma unroll
                for (int s0 = 0; s0 < 3; ++s0) {
                    u32 s = (u32)s0;
                    for (int j = 0; j < nvalid; ++j) s = s == 0 ? ((z >> j) & 1u) : (s == 1 ? 2u : 0u);
                    ex3[s0] = s;
                }
            }
        }
        u32 f = ex3[0] | (ex3[1] << 2) | (ex3[2] << 4);
        u32 fex;                                    // map of the wave's bytes before this lane
        if (__all(fn_const(f))) {                   // the usual wave: the neighbour's (constant) map is the map of all before
            fex = (u32)__shfl_up((int)f, 1, 64);
            if (lane == 0) fex = FN_IDENT;
            if (lane == 63) sh.wfn[wv] = f;
        } else {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u32 y = (u32)__shfl_up((int)f, d, 64);
                if (lane >= d) f = fn_compose(y, f);
            }
            if (lane == 63) sh.wfn[wv] = f;
            fex = (u32)__shfl_up((int)f, 1, 64);
            if (lane == 0) fex = FN_IDENT;
        }
        lds_barrier();
        u32 wcar = FN_IDENT, ftile = FN_IDENT;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < wv) wcar = fn_compose(wcar, sh.wfn[q]);
            ftile = fn_compose(ftile, sh.wfn[q]);
        }
        const u32 fpre = fn_compose(wcar, fex);     // map of all bytes of the tile before this lane

        // ---- the sums: one when the entry state is known (uniform), else one per entry state -----------------------------
        const bool known = fn_const(fprev);
        const u32 s_in = fprev & 3u;
        const int n_sums = known ? 1 : 3;
        for (int s = 0; s < n_sums; ++s) {
            const u32 es = fn_apply(fpre, known ? s_in : (u32)s);
            const u32 tot = dpp_scan_add(rlm_lane_sum(st3, wp, z, vm, es));
            if (lane == 63) sh.wsum[s][wv] = tot;
        }
        lds_barrier();
        if (tid == 0) {
            u32 sum[3], map = ftile;
#pragma unroll
            for (int s = 0; s < 3; ++s) sum[s] = sh.wsum[s][0] + sh.wsum[s][1] + sh.wsum[s][2] + sh.wsum[s][3];
            if (known) {
                map = fn_apply(ftile, s_in) * 0x15u;
                sum[1] = sum[2] = sum[0];
            }
            gstore<uint4>(rec + t, make_uint4(map, sum[0], sum[1], sum[2]));
        }
        // the next tile writes wfn after this barrier and wsum after its own first one: thread 0 has read both by then
    }
}

// (A then B) of {map, sum per entry state}
struct RlmAgg {
    u32 f;
    u64 s[3];
};
__device__ __forceinline__ RlmAgg rlm_then(const RlmAgg &a, const RlmAgg &b)
{
    RlmAgg r;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const u32 m = fn_apply(a.f, (u32)e);
        r.s[e] = a.s[e] + (m == 0 ? b.s[0] : m == 1 ? b.s[1] : b.s[2]);
    }
    r.f = fn_compose(a.f, b.f);
    return r;
}

__global__ __launch_bounds__(RLD_THREADS) void rle_measure_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                                  int nblk, const u64 *__restrict__ d_in_n,
                                                                  const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                                                  int *__restrict__ err)
{
    __shared__ u32 wf[4];
    __shared__ u64 ws[4][3];
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
        const u32 nt = (u32)((n + RLD_TILE - 1) / RLD_TILE);
        const uint4 *r = rec + tbase[b];
        const u32 per = (nt + RLD_THREADS - 1) / RLD_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        RlmAgg a = {FN_IDENT, {0, 0, 0}};
        for (u32 j = lo; j < hi; ++j) {
            const uint4 v = gload<uint4>(r + j);
            const RlmAgg t = {v.x, {v.y, v.z, v.w}};
            a = rlm_then(a, t);
        }
        // ordered reduction: after the step of distance d lane l holds lanes [l, l + 2 d) of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            RlmAgg o;
            o.f = (u32)__shfl_down((int)a.f, d, 64);
#pragma unroll
            for (int e = 0; e < 3; ++e) o.s[e] = (u64)__shfl_down((unsigned long long)a.s[e], d, 64);
            if (lane + d < 64) a = rlm_then(a, o);
        }
        if (lane == 0) {
            wf[wv] = a.f;
            ws[wv][0] = a.s[0]; ws[wv][1] = a.s[1]; ws[wv][2] = a.s[2];
        }
        lds_barrier();
        if (tid == 0) {
            u32 s = 0;
            u64 total = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                total += ws[q][s];
                s = fn_apply(wf[q], s);
            }
            // a stream that ends inside a triple, or more output than any block may have: both are the oracle's code
            const bool bad = s != 0 || total > (u64)SHAFA_RLE_DECODE_MAX;
            if (bad) set_error(err + b, SHAFA_FILE_UNRECOGNIZABLE);
            d_out_n[b] = bad ? 0 : total;
        }
        lds_barrier();                              // the next block of this workgroup writes wf / ws
    }
}

}  // namespace

int rlemeasure_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                          const u64 *d_in_n, u64 *d_out_n)
{
    u64 ntiles = 0;
    for (int b = 0; b < nblocks; ++b) ntiles += ceil_div_u64(h_in_cap[b], RLD_TILE);
    if (ntiles > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    // workspace: the tile records, then what the host uploads: offsets, capacities, first tile numbers
    const size_t nb = (size_t)nblocks;
    size_t off = 0;
    const size_t o_rec = off; off += (size_t)ntiles * 16;
    const size_t o_up = off;
    const size_t u_off = 0, u_cap = nb * 8, u_base = 2 * nb * 8, up_bytes = (2 * nb * 8 + (nb + 1) * 4 + 15) & ~(size_t)15;
    off += up_bytes;
    int rc = batch_reserve(bt, st, off);
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
        base += (u32)ceil_div_u64(h_in_cap[b], RLD_TILE);
    }
    hb[nblocks] = base;
    memset(hs + u_base + (nb + 1) * 4, 0, up_bytes - (u_base + (nb + 1) * 4));
    if ((rc = batch_upload(bt, st, ws + o_up, hs, up_bytes))) return rc;
    const u64 *d_off = (const u64 *)(ws + o_up + u_off), *d_cap = (const u64 *)(ws + o_up + u_cap);
    const u32 *d_base = (const u32 *)(ws + o_up + u_base);
    if (ntiles) {
        const u32 nt = (u32)ntiles, per_wg = (nt + RLM_MAX_WGS - 1) / RLM_MAX_WGS, wgs = (nt + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(rle_measure_tiles, dim3(wgs), dim3(RLD_THREADS), 0, st, d_in, d_off, d_cap, d_base, nblocks, d_in_n,
                           (uint4 *)(ws + o_rec), nt, per_wg);
    }
    const u32 bw = (u32)nblocks < RLM_MAX_BLOCK_WGS ? (u32)nblocks : RLM_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(rle_measure_blocks, dim3(bw), dim3(RLD_THREADS), 0, st, d_cap, d_base, nblocks, d_in_n,
                       (const uint4 *)(ws + o_rec), d_out_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
