// crc32.hip — CRC-32 (zlib / PNG / gzip: polynomial 0xEDB88320 reflected, init and final XOR 0xFFFFFFFF) of byte regions in
// device memory (shafa_hipd_crc32_dev) and of concatenations, from finished CRCs and lengths alone (shafa_hipd_crc32_combine_dev).
//
// A region is block b's d_in_n[b] bytes at d_in + in_off[b], at ANY byte alignment, and no copy of it is made: a lane reads
// the aligned 16-byte words around the 32 bytes it wants and shifts them into place (shift_words, as compare.hip does for
// its ref side).  Such a word is only read when it holds at least one byte of the region, and bytes behind d_in_n[b] are
// masked to zero before they count.
//
// The arithmetic.  A 32-bit value is a polynomial over GF(2) mod P, bit 31 = x^0 (the reflected form zlib keeps).  With
// init 0 and no final XOR the CRC of M is raw(M) = M(x) x^32 mod P: linear, raw(A || B) = raw(A) x^(8 |B|) ^ raw(B), leading
// zero bytes are free, and the init word is the same as 0xFFFFFFFF XORed into the message's first four bytes.  gfx950 has no
// carry-less multiply, so a product is 32 AND / XOR steps; the passes keep them few and their right operands constant:
//   crc32_tiles   every 8 KiB tile, ZERO PADDED to the full tile so that every place is a constant -> one 16-byte record, a
//                 word per wave.  A lane digests its 32 bytes word by word through eight 16-entry nibble tables in LDS, each
//                 entry stored 32 times, once per bank: lane l reads copy l mod 32, so the 32 lanes of a ds_read_b32 group hit
//                 32 different banks whatever the data (256-entry byte tables would cost one look-up less per byte and ~3.5
//                 conflict cycles more on random bytes).  Then ONE product puts the lane in its place, by the constant
//                 x^(256 (255 - tid)) whose 32 multiples K x^i the lane keeps in registers (3 instructions a bit), and the wave
//                 XORs its lanes together.  The four waves never meet after the prologue: no barrier in the tile loop.
//   crc32_blocks  one workgroup per block.  The block's records, right aligned on 256 runs of equal length (leading zero
//                 records are free): Horner over a thread's run by the constant x^65536, the thread's place x^(65536 per (255 -
//                 tid)) as products by the constants x^(2^k), an XOR reduction, and thread 0 takes the z < 8192 pad bytes of
//                 the last tile off again with x^(-8 z) — x is invertible mod P — as products by the constants x^(-8 2^k),
//                 k < 13.  The alternative, a general exponent for the partial tile inside crc32_tiles, would put a second, data
//                 dependent place product and its branch into the loop every other tile runs through.
//   crc32_combine one workgroup per file: thread t raises x^8 to the bytes after its block (a scan of the lengths from the
//                 file's end, 256 blocks a round) by the same constant products, then an XOR reduction.  The rule holds on
//                 finished CRCs: the conditioning cancels (zlib's crc32_combine).
// Every product's right operand is a row of crc_rows: 32 consecutive multiples C x^i of a constant C, built at compile time.
// No workgroup waits for another, no atomics, the result does not depend on scheduling.
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr u32 CRC_POLY = 0xEDB88320u;
constexpr u32 CRC_ONE = 0x80000000u;                 // x^0
constexpr u32 CRC_ORDER = 0xFFFFFFFFu;               // P is primitive: x^(2^32 - 1) = 1

__host__ __device__ constexpr u32 crc_times_x(u32 a) { return (a >> 1) ^ ((a & 1u) ? CRC_POLY : 0u); }
constexpr u32 crc_mul(u32 a, u32 b)
{
    u32 p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (CRC_ONE >> i)) p ^= b;
        b = crc_times_x(b);
    }
    return p;
}
constexpr u32 crc_x_pow(u64 e)
{
    u32 r = CRC_ONE, s = CRC_ONE >> 1;
    for (; e; e >>= 1) {
        if (e & 1) r = crc_mul(r, s);
        s = crc_mul(s, s);
    }
    return r;
}

// rows of 32 multiples C x^i: 0 .. 31: C = x^(2^k); 32 .. 44: C = x^(-8 2^k), k < 13 (a tile's pad is below 2^13 bytes)
constexpr int CRC_ROW_TILE = 16;                     // x^65536: one 8 KiB tile further
constexpr int CRC_ROW_UNPAD = 32;
constexpr int CRC_UNPAD_BITS = 13;
constexpr int CRC_ROWS = CRC_ROW_UNPAD + CRC_UNPAD_BITS;
static_assert((1 << CRC_UNPAD_BITS) == TP_TILE, "the pad of a tile takes CRC_UNPAD_BITS bits");
static_assert(8ull * TP_TILE == 1ull << CRC_ROW_TILE, "CRC_ROW_TILE is one tile's bits");
struct CrcRows {
    u32 m[CRC_ROWS][32];
};
constexpr CrcRows crc_make_rows()
{
    CrcRows t = {};
    u32 c = CRC_ONE >> 1;
    for (int k = 0; k < 32; ++k) {
        u32 v = c;
        for (int i = 0; i < 32; ++i, v = crc_times_x(v)) t.m[k][i] = v;
        c = crc_mul(c, c);
    }
    c = crc_x_pow((u64)CRC_ORDER - 8);
    for (int k = 0; k < CRC_UNPAD_BITS; ++k) {
        u32 v = c;
        for (int i = 0; i < 32; ++i, v = crc_times_x(v)) t.m[CRC_ROW_UNPAD + k][i] = v;
        c = crc_mul(c, c);
    }
    return t;
}
// lane places of a tile: thread t's 32 bytes are followed by 255 - t lanes of 256 bits
struct CrcLanes {
    u32 k[TP_THREADS];
};
constexpr CrcLanes crc_make_lanes()
{
    CrcLanes t = {};
    const u32 step = crc_x_pow(8 * TP_BPL);
    u32 c = CRC_ONE;
    for (int l = TP_THREADS - 1; l >= 0; --l) {
        t.k[l] = c;
        c = crc_mul(c, step);
    }
    return t;
}
__constant__ CrcRows crc_rows = crc_make_rows();
__constant__ CrcLanes crc_lanes = crc_make_lanes();

// the rule, stated on known values (zlib's x2n_table; the check value of "123456789" is the GPU tests')
static_assert(crc_x_pow(32) == CRC_POLY && crc_x_pow(1ull << 6) == 0xb1e6b092u && crc_x_pow(1ull << 31) == 0xc4e22c3cu,
              "x^(2^k) mod P");
static_assert(crc_x_pow(CRC_ORDER) == CRC_ONE && crc_x_pow(1ull << 32) == CRC_ONE >> 1, "the order of x divides 2^32 - 1");
static_assert(crc_mul(crc_x_pow((u64)CRC_ORDER - 8), crc_x_pow(8)) == CRC_ONE, "x^(-8) x^8 = 1");
static_assert(crc_mul(crc_x_pow((u64)CRC_ORDER - 8 * 4096ull), crc_x_pow(8 * 4096)) == CRC_ONE, "x^(-8 2^12)");

// e mod 2^32 - 1, or 2^32 - 1 itself, which serves as well: x^(2^32 - 1) = 1
__device__ __forceinline__ u32 crc_exp_mod(u64 e)
{
    e = (e & 0xFFFFFFFFull) + (e >> 32);             // <= 2^33 - 2
    e = (e & 0xFFFFFFFFull) + (e >> 32);             // <= 2^32 - 1
    return (u32)e;
}

// a C for the row of C's multiples (uniform): 3 instructions a bit
__device__ __forceinline__ u32 crc_mul_row(u32 a, const u32 *__restrict__ row)
{
    u32 p = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) p ^= row[i] & (u32)((int)(a << i) >> 31);
    return p;
}

// a x^e: a product by x^(2^k) for every bit k of e (a loop round is skipped by a wave none of whose lanes has the bit)
__device__ __forceinline__ u32 crc_mul_x_pow(u32 a, u32 e)
{
#pragma unroll 1
    for (int k = 0; k < 32; ++k) {
        if (__builtin_amdgcn_readfirstlane((int)(__ballot(e >> k) == 0))) break;
        if ((e >> k) & 1u) a = crc_mul_row(a, crc_rows.m[k]);
    }
    return a;
}

// ---- the tiles kernel ---------------------------------------------------------------------------------------------------
constexpr int CRC_NIB = 8 * 16;                      // nibble tables of a word: entry (j, v) = the 32 steps from v << 4 j
constexpr int CRC_COPIES = 32;                       // one per LDS bank

// The lane's 32 bytes of the tile at pos0 of a block of n bytes at src (sh = src mod 16 = 4 Q + r), little-endian in w; the
// bytes behind n are 0.  The aligned word at s16 holds byte p of the block; the next two are read where they start in front
// of the block's end (the third is wanted only when src is not 16-aligned).
template <int Q>
__device__ __forceinline__ void crc_lane_load(const u8 *src, u64 n, u64 pos0, u32 r, u32 (&w)[8])
{
    const u32 sh = 4u * Q + r;
    const u64 p = pos0 + (u64)threadIdx.x * TP_BPL;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = 0;
    if (p >= n) return;
    const u8 *s16 = (const u8 *)(((u64)(uintptr_t)src + p) & ~(u64)15);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 a = gload_nt<uint4>(s16);
    uint4 b = zero, c = zero;
    if (p + 16 - sh < n) b = gload_nt<uint4>(s16 + 16);
    if (sh != 0 && p + 32 - sh < n) c = gload_nt<uint4>(s16 + 32);
    const uint4 v0 = sh == 0 ? a : shift_words<Q>(a, b, r), v1 = sh == 0 ? b : shift_words<Q>(b, c, r);
    w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
    const u64 left = n - p;
    if (left < TP_BPL) {                             // the block's last lane: slack, or a neighbour's bytes, behind it
        const u32 nv = (u32)left;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u32 keep = nv > 4u * i ? nv - 4u * i : 0u;
            w[i] &= keep >= 4 ? 0xFFFFFFFFu : (1u << (8 * keep)) - 1u;
        }
    }
}

// c after 32 more steps: the XOR of its eight nibbles' entries
__device__ __forceinline__ u32 crc_word(const u32 *nib, u32 copy, u32 c)
{
    u32 o = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) o ^= nib[(16 * j + ((c >> (4 * j)) & 15u)) * CRC_COPIES + copy];
    return o;
}

__global__ __launch_bounds__(TP_THREADS) void crc32_tiles(const u8 *__restrict__ d_in, const u64 *__restrict__ in_off,
                                                          const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                                          const u64 *__restrict__ d_in_n, uint4 *__restrict__ rec, u32 n_tiles,
                                                          u32 per_wg)
{
    __shared__ u32 nib[CRC_NIB * CRC_COPIES];
    __shared__ u32 uniq[CRC_NIB];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    if (tid < CRC_NIB) {
        u32 s = (u32)(tid & 15) << (4 * (tid >> 4));
        for (int i = 0; i < 32; ++i) s = crc_times_x(s);
        uniq[tid] = s;
    }
    lds_barrier();
    for (int i = tid; i < CRC_NIB * CRC_COPIES; i += TP_THREADS) nib[i] = uniq[i / CRC_COPIES];
    lds_barrier();
    u32 place[32];                                   // K x^i, K = this thread's place in a tile
    place[0] = crc_lanes.k[tid];
#pragma unroll
    for (int i = 1; i < 32; ++i) place[i] = crc_times_x(place[i - 1]);
    const u32 copy = (u32)lane & (CRC_COPIES - 1);
    for (TpWalk wk(d_in, in_off, in_cap, tbase, nblk, d_in_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        u32 w[8];
        switch (sh >> 2) {                           // uniform
        case 0: crc_lane_load<0>(wk.in, wk.n, wk.pos0, r, w); break;
        case 1: crc_lane_load<1>(wk.in, wk.n, wk.pos0, r, w); break;
        case 2: crc_lane_load<2>(wk.in, wk.n, wk.pos0, r, w); break;
        default: crc_lane_load<3>(wk.in, wk.n, wk.pos0, r, w); break;
        }
        if (wk.k == 0 && tid == 0) w[0] ^= 0xFFFFFFFFu;          // the init word, on the padded tile's first four bytes
        u32 c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) c = crc_word(nib, copy, c ^ w[j]);
        u32 p = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) p ^= place[i] & (u32)((int)(c << i) >> 31);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) p ^= (u32)__shfl_xor((int)p, d, 64);
        if (lane == 0) gstore<u32>((u32 *)rec + 4ull * wk.t + (u32)wv, p);
    }
}

// ---- the blocks kernel --------------------------------------------------------------------------------------------------
// tp_launch's signature: d_out is the call's d_crc, 32 bits a block
__global__ __launch_bounds__(TP_THREADS) void crc32_blocks(const u64 *__restrict__ in_cap, const u32 *__restrict__ tbase, int nblk,
                                                           const u64 *__restrict__ d_in_n, const uint4 *__restrict__ rec,
                                                           u64 *__restrict__ d_out, int *__restrict__ err)
{
    __shared__ u32 wacc[TP_THREADS / 64];
    u32 *d_crc = (u32 *)d_out;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_in_n[b];
        if (n > in_cap[b] || n == 0) {              // (uniform) past the block's region, or the empty message
            if (tid == 0) {
                if (n) set_error(err + b, SHAFA_OUTSIDE_MODULE);
                d_crc[b] = 0;
            }
            continue;
        }
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        const uint4 *r = rec + tbase[b];
        // 256 runs of `per` records that end with the block's last one; the first `lead` are not there
        const u32 per = (nt + TP_THREADS - 1) / TP_THREADS;
        const u64 lead = (u64)per * TP_THREADS - nt;
        u32 a = 0;
        for (u32 i = 0; i < per; ++i) {
            const u64 v = (u64)tid * per + i;
            if (v < lead) continue;
            const uint4 t = gload<uint4>(r + (v - lead));
            a = crc_mul_row(a, crc_rows.m[CRC_ROW_TILE]) ^ t.x ^ t.y ^ t.z ^ t.w;
        }
        // the run is followed by 255 - tid runs of per tiles
        a = crc_mul_x_pow(a, a ? crc_exp_mod((8ull * TP_TILE) * per * (u64)(TP_THREADS - 1 - tid)) : 0u);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) a ^= (u32)__shfl_xor((int)a, d, 64);
        if (lane == 0) wacc[wv] = a;
        lds_barrier();
        if (tid == 0) {
            u32 c = wacc[0];
#pragma unroll
            for (int q = 1; q < TP_THREADS / 64; ++q) c ^= wacc[q];
            const u32 z = (u32)((u64)nt * TP_TILE - n);         // the last tile's pad
#pragma unroll 1
            for (int k = 0; k < CRC_UNPAD_BITS; ++k)
                if ((z >> k) & 1u) c = crc_mul_row(c, crc_rows.m[CRC_ROW_UNPAD + k]);
            d_crc[b] = ~c;
        }
        lds_barrier();                              // the next block of this workgroup writes the wave results
    }
}

// ---- the combine --------------------------------------------------------------------------------------------------------
constexpr int CRC_COMBINE_THREADS = 256;
constexpr u32 CRC_COMBINE_MAX_WGS = 1u << 20;

__global__ __launch_bounds__(CRC_COMBINE_THREADS) void crc32_combine_files(const int *__restrict__ first, const int *__restrict__ count,
                                                                           int nfiles, const u32 *__restrict__ d_crc,
                                                                           const u64 *__restrict__ d_n, u32 *__restrict__ d_file_crc,
                                                                           u64 *__restrict__ d_file_n)
{
    __shared__ u64 wsum[CRC_COMBINE_THREADS / 64];
    __shared__ u32 wacc[CRC_COMBINE_THREADS / 64];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    for (int f = blockIdx.x; f < nfiles; f += gridDim.x) {
        const int b0 = first[f], cnt = count[f];
        u64 after = 0;                               // bytes of the file behind the round's blocks
        u32 acc = 0;
        for (int done = 0; done < cnt; done += CRC_COMBINE_THREADS) {      // (uniform) from the file's end, thread 0 last
            const int i = cnt - 1 - done - tid;
            const bool on = i >= 0;
            const u64 len = on ? d_n[(size_t)b0 + (size_t)(on ? i : 0)] : 0ull;
            const u64 incl = wave_incl_scan_add<u64>(len);
            if (lane == 63) wsum[wv] = incl;
            lds_barrier();
            u64 s = after + incl - len;              // the bytes after this thread's block
            u64 total = 0;
#pragma unroll
            for (int q = 0; q < CRC_COMBINE_THREADS / 64; ++q) {
                if (q < wv) s += wsum[q];
                total += wsum[q];
            }
            const u32 c = on ? d_crc[(size_t)b0 + (size_t)(on ? i : 0)] : 0u;
            acc ^= crc_mul_x_pow(c, c ? crc_exp_mod(8ull * crc_exp_mod(s)) : 0u);
            after += total;
            lds_barrier();                          // the next round writes the wave sums
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc ^= (u32)__shfl_xor((int)acc, d, 64);
        if (lane == 0) wacc[wv] = acc;
        lds_barrier();
        if (tid == 0) {
            u32 c = wacc[0];
#pragma unroll
            for (int q = 1; q < CRC_COMBINE_THREADS / 64; ++q) c ^= wacc[q];
            d_file_crc[f] = c;
            d_file_n[f] = after;
        }
        lds_barrier();
    }
}

}  // namespace

// workspace: tp_launch's (16 B per tile of the capacities, then the per-block upload).  The caller has checked that the
// tiles number fewer than 2^31.
int crc32_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, u32 *d_crc)
{
    return tp_launch(crc32_tiles, crc32_blocks, bt, st, nblocks, d_in, h_in_off, h_in_cap, d_in_n, (u64 *)d_crc);
}

// workspace: [first][count], what the host uploads
int crc32_combine_launch_dev(Batch *bt, hipStream_t st, int nfiles, const int *h_first, const int *h_count, const u32 *d_crc,
                             const u64 *d_n, u32 *d_file_crc, u64 *d_file_n)
{
    const size_t nf = (size_t)nfiles, up_bytes = (2 * nf * 4 + 15) & ~(size_t)15;
    int rc = batch_reserve(bt, st, up_bytes);
    if (rc) return rc;
    u8 *hs = (u8 *)batch_stage(bt, st, up_bytes);
    if (!hs) return SHAFA_LACK_OF_MEMORY;
    memcpy(hs, h_first, nf * 4);
    memcpy(hs + nf * 4, h_count, nf * 4);
    memset(hs + 2 * nf * 4, 0, up_bytes - 2 * nf * 4);
    if ((rc = batch_upload(bt, st, bt->d_ws, hs, up_bytes))) return rc;
    const int *d_first = (const int *)bt->d_ws, *d_count = d_first + nf;
    const u32 wgs = (u32)nfiles < CRC_COMBINE_MAX_WGS ? (u32)nfiles : CRC_COMBINE_MAX_WGS;
    hipLaunchKernelGGL(crc32_combine_files, dim3(wgs), dim3(CRC_COMBINE_THREADS), 0, st, d_first, d_count, nfiles, d_crc, d_n,
                       d_file_crc, d_file_n);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
