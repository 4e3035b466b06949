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
// The tile walk, the lane's load, the blocks kernel's skeleton and the launcher are tile_pass.hpp's, shared with the encoded-size
// pass; this file holds the summary.  The tiles of all blocks are numbered consecutively and dealt to the workgroups in equal
// runs, so one 64 MiB block next to thousands of small ones costs its own tiles and theirs, not their product.
//
// Algorithmic HBM bytes per block: rle_n read, 16 bytes per 8 KiB tile written and read again.
#include "common.hpp"
#include "internal.hpp"
#include "rld_fsm.hpp"
#include "tile_pass.hpp"

namespace {

struct RlmShared {
    u32 fsm[256];
    u32 wfn[4];
    u32 wsum[3][4];
};

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

__global__ __launch_bounds__(TP_THREADS) void rle_measure_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                                const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                                int nblk, const u64 *__restrict__ d_in_n,
                                                                uint4 *__restrict__ rec, u32 n_tiles, u32 per_wg)
{
    __shared__ __attribute__((aligned(16))) RlmShared sh;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    // before the walk knows whether the workgroup has a tile (the launcher starts none without): every thread gets here
    sh.fsm[tid] = g_rld_fsm.v[tid];
    lds_barrier();
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        // ---- the lane's 32 bytes, their zero mask, and the bytes with 0 replaced by 1 (a count of 0 acts as 1) ----------
        u32 w[8];
        const u32 nvalid = tp_lane_load(wk.in, wk.pos0, wk.n, w);
        // the map of the 32 bytes in front of the tile (one address for all lanes): constant nearly always, and then its
        // value IS the state the tile is entered in.  Tile 0 is entered in S0.
        u32 fprev = 0;
        if (wk.k > 0) {
            const uint4 p0 = gload<uint4>(wk.in + wk.pos0 - 32), p1 = gload<uint4>(wk.in + wk.pos0 - 16);
            const u32 pw[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            u32 pst[3], pex[3];
            fsm32(sh.fsm, zmask32(pw), pst, pex);
            fprev = pex[0] | (pex[1] << 2) | (pex[2] << 4);
        }
        const u32 vm = nvalid >= 32u ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
        const u32 z = zmask32(w) & vm;
        u32 wp[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wp[i] = w[i] | (zero_bytes80(w[i]) >> 7);

        // ---- the lane's map; bytes past the end of the block do not move the state ---------------------------------------
        u32 st3[3], ex3[3];
        if (__all(z == 0u && nvalid == (u32)TP_BPL)) {      // a wave without a zero byte: literals once the state is S0
            st3[0] = 0xFFFFFFFFu; st3[1] = 0xFFFFFFFCu; st3[2] = 0xFFFFFFFEu;
            ex3[0] = ex3[1] = ex3[2] = 0;
        } else {
            fsm32(sh.fsm, z, st3, ex3);
            if (nvalid < (u32)TP_BPL) {           // the table ran over 32 bytes: walk the valid ones (the block's last lane)
#pragma unroll
                for (int s0 = 0; s0 < 3; ++s0) {
                    u32 s = (u32)s0;
                    for (u32 j = 0; j < nvalid; ++j) s = s == 0 ? ((z >> j) & 1u) : (s == 1 ? 2u : 0u);
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
            gstore<uint4>(rec + wk.t, make_uint4(map, sum[0], sum[1], sum[2]));
        }
        // the next tile writes wfn after this barrier and wsum after its own first one: thread 0 has read both by then
    }
}

// the blocks kernel's four wave results: touched by RlmSum's put and finish only, which tp_blocks calls between its two barriers
__shared__ u32 rlm_wf[4];
__shared__ u64 rlm_ws[4][3];

// the blocks kernel's summary: {map, sum per entry state}, (A then B) as above
struct RlmSum {
    struct Agg {
        u32 f;
        u64 s[3];
    };
    static __device__ __forceinline__ Agg identity() { return {FN_IDENT, {0, 0, 0}}; }
    static __device__ __forceinline__ Agg read(const uint4 &v) { return {v.x, {v.y, v.z, v.w}}; }
    static __device__ __forceinline__ Agg then(const Agg &a, const Agg &b)
    {
        Agg r;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const u32 m = fn_apply(a.f, (u32)e);
            r.s[e] = a.s[e] + (m == 0 ? b.s[0] : m == 1 ? b.s[1] : b.s[2]);
        }
        r.f = fn_compose(a.f, b.f);
        return r;
    }
    static __device__ __forceinline__ Agg from_lane(const Agg &a, int d)
    {
        Agg o;
        o.f = (u32)__shfl_down((int)a.f, d, 64);
#pragma unroll
        for (int e = 0; e < 3; ++e) o.s[e] = (u64)__shfl_down((unsigned long long)a.s[e], d, 64);
        return o;
    }
    static __device__ __forceinline__ void put(int q, const Agg &a)
    {
        rlm_wf[q] = a.f;
        rlm_ws[q][0] = a.s[0]; rlm_ws[q][1] = a.s[1]; rlm_ws[q][2] = a.s[2];
    }
    // a block is entered in S0: that state's sums, wave after wave.  A stream that ends inside a triple (exit state not S0),
    // or more output than any block may have: both are the oracle's code
    static __device__ __forceinline__ int finish(u64 &size)
    {
        u32 s = 0;
        u64 total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            total += rlm_ws[q][s];
            s = fn_apply(rlm_wf[q], s);
        }
        const bool bad = s != 0 || total > (u64)SHAFA_RLE_DECODE_MAX;
        size = bad ? 0 : total;
        return bad ? SHAFA_FILE_UNRECOGNIZABLE : 0;
    }
};

__global__ __launch_bounds__(TP_THREADS) void rle_measure_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase,
                                                                 int nblk, const u64 *__restrict__ d_in_n,
                                                                 const uint4 *__restrict__ rec, u64 *__restrict__ d_out_n,
                                                                 int *__restrict__ err)
{
    tp_blocks<RlmSum>(in_cap, tbase, nblk, d_in_n, rec, d_out_n, err);
}

}  // namespace

int rlemeasure_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                          const u64 *d_in_n, u64 *d_out_n)
{
    return tp_launch(rle_measure_tiles, rle_measure_blocks, bt, st, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_out_n);
}
