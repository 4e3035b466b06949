// records.hip — fixed-width records <-> one byte string per byte of the record (shafa_hipd_split_records_dev,
// shafa_hipd_merge_records_dev): planes.hip's transposes for ANY width W = 1 .. SHAFA_RECORDS_MAX_WIDTH, a run-time argument.
//
// Block b is d_n[b] (<= cap[b]) records of W bytes.  RECORD SIDE: its W d_n[b] bytes at d_rec + off[b], at ANY byte alignment,
// never copied.  COLUMN SIDE: column j (byte j of every record) is d_n[b] bytes at d_planes + poff[b W + j], every one a
// multiple of 16.  At W = 1, 2, 4, 8 the bytes are the plain plane entries'.
//
// planes.hip transposes in registers, which needs a power-of-two element that a lane's 16-byte words hold whole.  Here the
// transposition goes through LDS.  A tile is tile_pass.hpp's (TpWalk, 8192 RECORDS, numbered from the capacities, dealt to the
// workgroups in equal runs; an empty tile exits); a workgroup takes it in passes of P = SHAFA_RECORDS_PASS(W) records, whose
// P W <= 32 KiB bytes are one LDS IMAGE: the aligned 16-byte words of global memory that hold the pass's bytes, as they are, so
// image byte a is the byte at (the pass's first word) + a and record r's byte j is image byte sh + r W + j, sh = (the pass's
// address) mod 16.  Alignment costs an addition.
//   split   the image's words are loaded coalesced and streamed (lane l word l, l + 256, ..), stored to LDS; then a lane takes a
//           UNIT — 16 records of one column: 16 single-byte LDS reads, W bytes apart — and stores them as one word of the column,
//           streamed.  Units are numbered column-major (unit u = column u / G, group u % G of the pass's G groups of 16), so a
//           wave's 64 stores are 1 KiB contiguous wherever it stays inside a column.
//   merge   the mirror image: a lane loads a unit's word of the column (streamed) and scatters its 16 bytes into the image;
//           then the image's words go to global memory coalesced and streamed, whole lines.  Words that lie wholly inside the
//           pass's bytes are stored whole; the first and the last word of a pass, where the region is unaligned, hold bytes of
//           the neighbouring pass (another workgroup's) or of memory outside the region, and go as single bytes.
// Bank conflicts: the lanes of a wave walk consecutive groups of one column, 16 W bytes = 4 W dwords apart: 8 banks of 32 for an
// odd W, ONE bank for a multiple of 8.  The image is therefore stored with one dword of padding behind every 16 W bytes
// (image byte a lies at LDS byte a + 4 (a / 16 W); 16 W is a multiple of 16, so an aligned word is never cut): neighbours are
// then 4 W + 1 dwords apart, an odd number, and 32 lanes hit 32 banks.  The quotients by W and by G are multiplications by a
// reciprocal.
//
// What the measurements settled (the losing variants are tools/experiments/records_variants.patch).  Without the
// padding both directions fall from 4.0 - 4.4 TB/s to 1.2 TB/s at W = 16 and 32 (a 32-way conflict: 64 LDS cycles an
// instruction) and to 2.3 TB/s at 12.  merge's record-side stores are whole lines here, unlike planes.hip's strided ones, and
// streamed they are 1 - 2 % faster than plain at W = 3, 12, 16, 32 and 5 % at 8 wherever the two builds ran in pairs on one box
// (one unpaired run was mixed).  The sub-dword LDS accesses cost what the dword ones do: ds_read_u8 2.3 - 2.6 cycles a
// wave-instruction and CU, ds_write_b8 4.4 - 4.7 (tools/ubench/lds_ops).
//
// One launch, no workgroup waits for another; the only atomic is the error word of a block with d_n[b] > cap[b], of which no
// byte is read or written.  Algorithmic HBM bytes: every record byte read once and written once.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr u32 RC_IMAGE = 32768;                    // the bytes of records a pass holds at the most
// the image's words (RC_IMAGE + 15 bytes of alignment), what a block's last group of 16 reads or writes behind its last record
// (15 records), and the padding: one dword per 16 W bytes, 2056 bytes at the most (W = 1 .. 4, P = 8192); rc_passes_fit checks
constexpr u32 RC_LDS_BYTES = 36864;
constexpr u32 RC_PAD = 4;                          // the padding behind every 16 W bytes of the image

constexpr bool rc_passes_fit()
{
    for (u32 w = 1; w <= SHAFA_RECORDS_MAX_WIDTH; ++w) {
        const u32 p = SHAFA_RECORDS_PASS(w), img = p * w + 15 + 15 * w;
        if (p % 16 || SHAFA_RECORDS_TILE % p || p * w > RC_IMAGE || img + 4 * (img / (16 * w) + 1) > RC_LDS_BYTES) return false;
    }
    return true;
}
static_assert(TP_TILE == SHAFA_RECORDS_TILE, "tile_pass.hpp's walk is used as it is");
static_assert(rc_passes_fit(), "every width's pass is whole groups of 16, divides the tile and fits the LDS image");

// x / d = rc_div(x, rc_magic(d)) wherever x d <= 2^20 and x <= 2^11 + 2^6: with m = 2^20 / d + 1 the product x m is below 2^32,
// and its error x (m d - 2^20) <= x d stays under one unit of the quotient.  The callers' pairs: (a word of the image <= 2049,
// W <= 64) and (a unit < W G, the pass's groups G), W G <= 2^11 and G <= 2^9.
__device__ __forceinline__ u32 rc_magic(u32 d) { return (1u << 20) / d + 1u; }
__device__ __forceinline__ u32 rc_div(u32 x, u32 m) { return (x * m) >> 20; }

// LDS byte of image byte a, a / 16 W = q
__device__ __forceinline__ u32 rc_at(u32 a, u32 q) { return a + RC_PAD * q; }

// one pass of one block: cnt records from record e0, at rec (the record side, any alignment)
struct RcPass {
    u8 *rec16;                                     // the aligned word that holds the pass's first byte
    u32 sh, nbytes, nw, groups, units;             // rec mod 16; cnt W; the image's words; ceil(cnt / 16); groups W
    __device__ __forceinline__ RcPass(const u8 *in, u64 e0, u32 cnt, u32 w)
    {
        const u8 *rec = in + e0 * w;
        sh = (u32)((uintptr_t)rec & 15u);
        rec16 = (u8 *)rec - sh;
        nbytes = cnt * w;
        nw = (sh + nbytes + 15u) >> 4;
        groups = (cnt + 15u) >> 4;
        units = groups * w;
    }
};

// the LDS bytes of a unit's 16 record bytes: unit u of the pass = column j, group g; byte i is image byte sh + (16 g + i) W + j,
// which lies in image row g or, from t = sh + j + i W >= 16 W on, in row g + 1 (t < 32 W)
struct RcUnit {
    u32 j, g, c, base;
    __device__ __forceinline__ RcUnit(u32 u, const RcPass &ps, u32 mg, u32 w)
    {
        j = rc_div(u, mg);
        g = u - j * ps.groups;
        c = ps.sh + j;
        base = g * (16u * w + RC_PAD);
    }
    __device__ __forceinline__ u32 at(int i, u32 w) const
    {
        const u32 t = c + (u32)i * w;
        return base + t + (t >= 16u * w ? RC_PAD : 0u);
    }
};

__global__ __launch_bounds__(TP_THREADS) void records_split(const u8 *__restrict__ d_rec, const u64 *__restrict__ off,
                                                            const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                            const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                            const u64 *__restrict__ d_poff, int *__restrict__ err, u32 n_tiles,
                                                            u32 per_wg, u32 w)
{
    __shared__ __attribute__((aligned(16))) u32 lds[RC_LDS_BYTES / 4];
    const u8 *lds8 = (const u8 *)lds;
    const u32 tid = threadIdx.x, pass = SHAFA_RECORDS_PASS(w), mw = rc_magic(w);
    for (TpWalk wk(d_rec, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * w;
        const u64 tile_end = wk.n - wk.pos0 > TP_TILE ? wk.pos0 + TP_TILE : wk.n;
#pragma nounroll
        for (u64 e0 = wk.pos0; e0 < tile_end; e0 += pass) {                // (uniform) the barriers are inside
            const RcPass ps(wk.in, e0, tile_end - e0 > pass ? pass : (u32)(tile_end - e0), w);
            // the image: four words a lane in flight
#pragma nounroll
            for (u32 k0 = tid; k0 < ps.nw; k0 += 4 * TP_THREADS) {
                uint4 v[4] = {};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (k0 + i * TP_THREADS < ps.nw) v[i] = gload_nt<uint4>(ps.rec16 + 16ull * (k0 + i * TP_THREADS));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const u32 k = k0 + i * TP_THREADS;
                    if (k < ps.nw) {
                        u32 *p = lds + (rc_at(16u * k, rc_div(k, mw)) >> 2);
                        p[0] = v[i].x; p[1] = v[i].y; p[2] = v[i].z; p[3] = v[i].w;
                    }
                }
            }
            lds_barrier();
            const u32 mg = rc_magic(ps.groups);
#pragma nounroll
            for (u32 u = tid; u < ps.units; u += TP_THREADS) {
                const RcUnit un(u, ps, mg, w);
                const u64 po = poff[un.j];
                u32 o[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i >> 2] |= (u32)lds8[un.at(i, w)] << (8 * (i & 3));
                const u64 r0 = e0 + 16ull * un.g;
                u8 *dst = d_planes + po + r0;
                const uint4 ov = make_uint4(o[0], o[1], o[2], o[3]);
                if (tile_end - r0 >= 16) gstore_nt<uint4>(dst, ov);        // 1 KiB a wave, whole lines: streamed
                else {                                                     // the block ends inside the group
                    const u32 c = (u32)(tile_end - r0);
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if ((u32)k < c) gstore<u8>(dst + k, tp_byte_of(ov, k));
                }
            }
            lds_barrier();                                                 // the next pass writes the image
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

__global__ __launch_bounds__(TP_THREADS) void records_merge(u8 *__restrict__ d_rec, const u64 *__restrict__ off,
                                                            const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                            const u64 *__restrict__ d_n, const u8 *__restrict__ d_planes,
                                                            const u64 *__restrict__ d_poff, int *__restrict__ err, u32 n_tiles,
                                                            u32 per_wg, u32 w)
{
    __shared__ __attribute__((aligned(16))) u32 lds[RC_LDS_BYTES / 4];
    u8 *lds8 = (u8 *)lds;
    const u32 tid = threadIdx.x, pass = SHAFA_RECORDS_PASS(w), mw = rc_magic(w);
    for (TpWalk wk(d_rec, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * w;
        const u64 tile_end = wk.n - wk.pos0 > TP_TILE ? wk.pos0 + TP_TILE : wk.n;
#pragma nounroll
        for (u64 e0 = wk.pos0; e0 < tile_end; e0 += pass) {                // (uniform) the barriers are inside
            const RcPass ps(wk.in, e0, tile_end - e0 > pass ? pass : (u32)(tile_end - e0), w);
            const u32 mg = rc_magic(ps.groups);
            // a unit's word of its column (the word holds a byte of the column; what it holds behind the block's last record
            // goes into the image behind the pass's bytes, which are not stored) -> 16 bytes of the image
#pragma nounroll
            for (u32 u = tid; u < ps.units; u += TP_THREADS) {
                const RcUnit un(u, ps, mg, w);
                const uint4 v = gload_nt<uint4>(d_planes + poff[un.j] + e0 + 16ull * un.g);
#pragma unroll
                for (int i = 0; i < 16; ++i) lds8[un.at(i, w)] = tp_byte_of(v, i);
            }
            lds_barrier();
#pragma nounroll
            for (u32 k = tid; k < ps.nw; k += TP_THREADS) {
                const u32 *p = lds + (rc_at(16u * k, rc_div(k, mw)) >> 2);
                const uint4 v = make_uint4(p[0], p[1], p[2], p[3]);
                const int lo = (int)(16u * k) - (int)ps.sh;                // the word's first byte in the pass
                u8 *dst = ps.rec16 + 16ull * k;
                if (lo >= 0 && (u32)lo + 16u <= ps.nbytes) gstore_nt<uint4>(dst, v);       // 1 KiB a wave, whole lines: streamed
                else {
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (lo + i >= 0 && (u32)(lo + i) < ps.nbytes) gstore<u8>(dst + i, tp_byte_of(v, i));
                }
            }
            lds_barrier();                                                 // the next pass writes the image
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

}  // namespace

// workspace: tile_setup's with one extra, the column offsets (width a block), and no scratch.  The caller has checked the
// arguments.
int records_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 width, bool merge, u8 *d_rec, const u64 *h_off, const u64 *h_cap,
                       const u64 *d_n, u8 *d_planes, const u64 *h_plane_off)
{
    const TileExtra x = {h_plane_off, (size_t)nblocks * width * 8};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, &x, 1, 0, 0, &a)) return rc;
    const u64 *poff = (const u64 *)a.extra[0];
    const u32 wgs = a.wgs ? a.wgs : 1;               // without a tile one workgroup still looks for blocks past a capacity of 0
    if (merge)
        hipLaunchKernelGGL(records_merge, dim3(wgs), dim3(TP_THREADS), 0, st, d_rec, a.off, a.cap, a.tbase, nblocks, d_n,
                           (const u8 *)d_planes, poff, bt->d_err, a.nt, a.per_wg, width);
    else
        hipLaunchKernelGGL(records_split, dim3(wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_rec, a.off, a.cap, a.tbase, nblocks, d_n,
                           d_planes, poff, bt->d_err, a.nt, a.per_wg, width);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
