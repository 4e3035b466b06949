// planes_lag.hip — byte planes of LAGGED differences (shafa_hipd_split_planes_lag_dev, shafa_hipd_merge_planes_lag_dev, DESIGN
// 7.26): planes.hip's differences with a distance in them.  Block b is d_n[b] (<= cap[b]) elements of E = 1, 2, 4 or 8 bytes,
// x[i] as unsigned little-endian integers, L = lag[b] >= 1 its lag (one a block, from the host):
//     d[i] = x[i] - x[i - L] mod 2^(8 E)   (x[i] = 0 for i < 0),   plane j = byte j of the zigzag fold of d[i]
// and back x[i] = x[i - L] + d[i]: the block seen as rows of L columns, a prefix sum down every column.  ELEMENT SIDE at multiples
// of E (the entries refuse anything else), PLANE SIDE at multiples of 16, as everywhere.  The host clamps L to the block's
// capacity: a lag at or past d_n[b] subtracts nothing, whatever its value.
//
// split: one launch over tile_pass.hpp's tiles, the plain split's direct path (16 elements a lane: E aligned words shifted into
// place, v_perm_b32, one word of each plane).  The "base" of a unit is the unit L elements in front of it in the block's own
// region, read the same way at an alignment of its own (lag_base: the region moved up by L elements), elements in front of the
// block zeroed; subtract, fold, store.  2 bytes of traffic per tensor byte, the second read of the region from L2 where L is
// small.
//
// merge: a chunk is G rows of a strip of W columns, one column a lane (LagGeom):
//     L >= 256   W = 256: a row of a strip is 256 consecutive elements, a lane walks its column down the chunk's rows;
//     L < 256    W = L, and the workgroup's 256 lanes are S = 256 / L segments of 32 rows each, so a round of 32 S rows is a
//                contiguous run of 32 S L (4097 .. 8192) elements; the segments' totals go through LDS.
// A chunk is m rounds of 32 S rows; m grows with the block so that it has about SHAFA_PLANES_LAG_ITEMS chunk-strips (items) and
// the column sums stay few.  Three launches at the most, the stream their only order, no workgroup ever waits for another:
//     planes_lag_sums    the column sums of every chunk but the one the block ends in, mod 2^(8 E), E bytes each
//     planes_lag_scan    exclusive prefixes down each column of the sums, a workgroup a run of 32 columns, 8 chunks a lane a round
//     planes_lag_merge   the elements, chunk by chunk on top of its prefix; in a strip of 256 columns a lane takes four columns
//                        and eight of a round's rows (lag_merge_wide): a dword of each plane, four elements a store
// A block whose rows fit one chunk has no sums, and where no block has any the first two launches are not made.  All three walk
// the tiles of the capacities (TpWalk) and deal a block's items (or column runs) to its tiles in equal runs, so the grid is the
// plain entries' whatever the lags.  The planes are read twice: 3 bytes of traffic per tensor byte.  The sums of block b lie at
// LAG_SUMS_TILE elements per tile of the capacities in front of it: NC L <= (cap / 16)(1 + 1 / 32) once there are two chunks.
//
// The GRID entries (shafa_hipd_split_planes_grid_dev, shafa_hipd_merge_planes_grid_dev) take up to three lags a block,
// d = (1 - S^L0)(1 - S^L1)(1 - S^L2) x, the differences along every lag in turn.  split: this file's split with one base unit per
// non-empty subset of the block's lags, subtracted or added (planes_grid_split).  merge: a first pass from the planes at the
// block's smallest lag — planes.hip's merge of differences where that is 1, else the three launches above — then per further lag
// the three launches above with the ELEMENTS as their source, in place (LagSrc).
//
// The GRID QUANT entries (shafa_hipd_split_planes_grid_quant_dev, shafa_hipd_merge_planes_grid_quant_dev) are the grid
// entries for float and double elements under an error bound.  split: the grid split with every loaded unit, the lane's own and
// every base, quantised to integer codes in registers first, and the elements whose restored value misses the bound recorded
// (planes_grid_quant_split).  merge: the grid merge's chain, then the codes -> values in place (planes_field_restore) and the
// recorded elements' own bits on top (planes_field_patch).
// shafa_hipd_hist_planes_grid_quant_dev is to the quantising split what shafa_hipd_hist_planes_grid_dev is to the grid
// split: the planes' histograms without the planes, and the outliers counted instead of recorded (planes_grid_quant_hist).
// The GRID ROUND entries (shafa_hipd_split_planes_grid_round_dev, shafa_hipd_merge_planes_grid_round_dev,
// shafa_hipd_hist_planes_grid_round_dev) are the three above with another quantiser: the element's mantissa rounded to
// `keep` bits, half to even, in integer arithmetic on its own bits, for elements of 2, 4 and 8 bytes (planes_grid_round_split,
// planes_round_restore, planes_grid_round_hist); the records, the patch pass and the histogram's composition are those entries'.
// The three splits and the histograms of the grid family are one tile walk (grid_tile) with three callables, the plain and the
// rounding histogram one kernel body (grid_hist), the two restore passes one walk (restore_tile).
#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"
#include "planes_arith.hpp"

#include <vector>

namespace {

constexpr u32 LAG_STRIP = SHAFA_PLANES_LAG_STRIP;               // columns of a strip: one a lane
constexpr u32 LAG_ROWS = SHAFA_PLANES_LAG_ROWS;                 // rows a lane holds in registers at a time
constexpr u32 LAG_ITEMS = SHAFA_PLANES_LAG_ITEMS;               // items a block is cut into before its chunks grow
constexpr u32 LAG_SUMS_TILE = SHAFA_PLANES_TILE / 8;            // column sums per tile of the capacities
constexpr u32 LAG_SCAN_COLS = 32, LAG_SCAN_PER = 8;             // the scan: columns of a run, chunks a lane a round
static_assert(LAG_STRIP == TP_THREADS && LAG_ROWS * LAG_STRIP == TP_TILE, "a round of a strip is a tile");

template <int E> struct ElT { using T = u32; };
template <> struct ElT<1> { using T = u8; };
template <> struct ElT<2> { using T = u16; };
template <> struct ElT<8> { using T = u64; };

// the form of a block of capacity cap >= 1 and lag 1 <= L <= cap (all uniform)
struct LagGeom {
    u64 L;
    u32 W, S;          // a strip's columns; the segments of rows the lanes are cut into (L >= 256: 1)
    u32 m;             // rounds of LAG_ROWS S rows a chunk
    u64 NS, G, NC, NI; // strips; rows of a chunk; chunks of the capacity; items = NS NC, item w = chunk w / NS, strip w % NS
    __host__ __device__ LagGeom(u64 cap, u64 lag) : L(lag)
    {
        W = L < LAG_STRIP ? (u32)L : LAG_STRIP;
        S = LAG_STRIP / W;
        NS = (L + W - 1) / W;
        const u64 g0 = (u64)LAG_ROWS * S, rows = (cap + L - 1) / L, i0 = NS * ((rows + g0 - 1) / g0);
        m = i0 / LAG_ITEMS > 1 ? (u32)(i0 / LAG_ITEMS) : 1u;
        G = g0 * m;
        NC = (rows + G - 1) / G;
        NI = NS * NC;
    }
};

// ---- split
template <int E>
__device__ __forceinline__ void sub_words(u32 (&w)[4 * E], const u32 (&b)[4 * E])
{
#pragma unroll
    for (int i = 0; i < 4 * E; ++i) {
        if (E == 8) {
            if (i & 1) {
                const u64 v = ((u64)w[i] << 32 | w[i - 1]) - ((u64)b[i] << 32 | b[i - 1]);
                w[i - 1] = (u32)v; w[i] = (u32)(v >> 32);
            }
        } else if (E == 4) w[i] -= b[i];
        else w[i] = pk_sub<E>(w[i], b[i]);
    }
}

template <int E>
__device__ __forceinline__ void add_words(u32 (&w)[4 * E], const u32 (&b)[4 * E])
{
#pragma unroll
    for (int i = 0; i < 4 * E; ++i) {
        if (E == 8) {
            if (i & 1) {
                const u64 v = ((u64)w[i] << 32 | w[i - 1]) + ((u64)b[i] << 32 | b[i - 1]);
                w[i - 1] = (u32)v; w[i] = (u32)(v >> 32);
            }
        } else if (E == 4) w[i] += b[i];
        else w[i] = pk_add<E>(w[i], b[i]);
    }
}

// wb = elements e0 - L .. e0 - L + 15 of the region of n elements at src, zero where the index is negative (e0 + 16 > L: at
// least one is not).  The region moved up by L elements is a region at an alignment of its own whose unit e0 these are; an
// aligned word is read only where it holds a byte of the real region in front of byte n E.
template <int E>
__device__ __forceinline__ void lag_base(const u8 *src, u64 n, u64 L, u64 e0, u32 (&wb)[4 * E])
{
    const u64 moved = (u64)(uintptr_t)src - L * E;
    const u32 sh = (u32)(moved & 15u), r = sh & 3u;
    const long long p = (long long)(e0 * E), first = (long long)(L * E), end = (long long)(n * E);
    const u8 *s16 = (const u8 *)(uintptr_t)((moved + (u64)p) & ~(u64)15);
    uint4 a[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        a[i] = make_uint4(0, 0, 0, 0);
        const long long lo = p + 16 * i - (long long)sh;
        if (lo + 16 > first && lo < end && (i < E || sh != 0)) a[i] = gload<uint4>(s16 + 16 * i);
    }
    switch (sh >> 2) {                               // uniform
    case 0: shift_into<E, 0, false>(a, r, wb); break;
    case 1: shift_into<E, 1, false>(a, r, wb); break;
    case 2: shift_into<E, 2, false>(a, r, wb); break;
    default: shift_into<E, 3, false>(a, r, wb); break;
    }
    if (L > e0) {                                    // the unit the block's first L elements end in
        const u32 zb = (u32)(L - e0) * E;            // its bytes in front of element L
#pragma unroll
        for (int i = 0; i < 4 * E; ++i) {
            if (4u * i + 4u <= zb) wb[i] = 0;
            else if (4u * i < zb) wb[i] &= ~0u << (8u * (zb - 4u * i));
        }
    }
}

template <int E, int Q>
__device__ __forceinline__ void split_tile_lag(const TpWalk &wk, u32 r, u64 L, u8 *d_planes, const u64 *poff)
{
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u64 e0 = wk.pos0 + (u64)u * PL_PASS + (u64)threadIdx.x * PL_UNIT;
        if (e0 >= wk.n) continue;
        u32 w[4 * E];
        {
            uint4 a[E + 1];
            load_words<E, true>(wk.in, wk.n * E, e0 * E, 4u * Q + r, a);
            shift_into<E, Q, false>(a, r, w);
        }
        if (e0 + PL_UNIT > L) {
            u32 wb[4 * E];
            lag_base<E>(wk.in, wk.n, L, e0, wb);
            sub_words<E>(w, wb);
        }
        zz_fold<E, 4 * E>(w);
        split_store<E>(w, wk.n, e0, d_planes, poff);
    }
}

template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_lag_split(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                               const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                               const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                               const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                               int *__restrict__ err, u32 n_tiles, u32 per_wg)
{
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        const u64 L = d_lag[wk.b];
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: split_tile_lag<E, 0>(wk, r, L, d_planes, poff); break;
        case 1: split_tile_lag<E, 1>(wk, r, L, d_planes, poff); break;
        case 2: split_tile_lag<E, 2>(wk, r, L, d_planes, poff); break;
        default: split_tile_lag<E, 3>(wk, r, L, d_planes, poff); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- the grid differences: d = (1 - S^L0)(1 - S^L1)(1 - S^L2) x, one base unit (a TAP) per non-empty subset of the
// block's used lags (lg[k] != 0), read by lag_base at the summed distance, subtracted for an odd subset and added for an even
// one; one base is live at a time.  A subset with an unused lag, or whose distance is past the unit, is skipped.
// grid_tile is the one walk of a tile for the grid split, its quantising and rounding forms and the three histograms, which
// differ in three callables only:
//     own(w, e0, c)    the lane's own unit from element e0 as loaded, c = min(16, n - e0) of its elements in front of the block's
//                      end: nothing, or the elements -> their codes with the first c judged
//     tap(wb)          a tap's unit: nothing, or the elements -> their codes (the zeros in front of the block stay zeros)
//     sink(w, e0, c)   the unit of differences: fold and store a word of each plane, or count the c elements' bytes
// Each member's tile function makes its lambdas from plain arguments BEHIND its kernel's switch over Q: built in front of one
// shared switch, the closures cost the splits their code (LABNOTES, "one grid tile walk").
template <int E, int Q, class Own, class Tap, class Sink>
__device__ __forceinline__ void grid_tile(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS], Own &&own, Tap &&tap,
                                          Sink &&sink)
{
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u64 e0 = wk.pos0 + (u64)u * PL_PASS + (u64)threadIdx.x * PL_UNIT;
        if (e0 >= wk.n) continue;
        u32 w[4 * E];
        {
            uint4 a[E + 1];
            load_words<E, true>(wk.in, wk.n * E, e0 * E, 4u * Q + r, a);
            shift_into<E, Q, false>(a, r, w);
        }
        const u32 c = wk.n - e0 >= PL_UNIT ? (u32)PL_UNIT : (u32)(wk.n - e0);
        own(w, e0, c);
#pragma nounroll
        for (u32 sub = 1; sub < 1u << SHAFA_PLANES_GRID_LAGS; ++sub) {          // (uniform)
            u64 dist = 0;
            bool used = true;
#pragma unroll
            for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k)
                if (sub >> k & 1u) {
                    used = used && lg[k] != 0;
                    dist += lg[k];
                }
            if (!used) continue;                     // (uniform)
            if (e0 + PL_UNIT > dist) {
                u32 wb[4 * E];
                lag_base<E>(wk.in, wk.n, dist, e0, wb);
                tap(wb);
                if (__builtin_popcount(sub) & 1) sub_words<E>(w, wb);           // (uniform)
                else add_words<E>(w, wb);
            }
        }
        sink(w, e0, c);
    }
}

// the grid split's tile: nothing is done to a loaded unit, the finished one is folded and stored
template <int E, int Q>
__device__ __forceinline__ void split_tile_grid(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS], u8 *d_planes,
                                                const u64 *poff)
{
    grid_tile<E, Q>(wk, r, lg, [](u32 (&)[4 * E], u64, u32) {}, [](u32 (&)[4 * E]) {}, [&](u32 (&w)[4 * E], u64 e0, u32) {
        zz_fold<E, 4 * E>(w);
        split_store<E>(w, wk.n, e0, d_planes, poff);
    });
}

// d_lag: SHAFA_PLANES_GRID_LAGS rows of nblk lags, clamped by the host: 0 where a slot is unused or at or past the capacity
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_split(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                                const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                                const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                                int *__restrict__ err, u32 n_tiles, u32 per_wg)
{
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: split_tile_grid<E, 0>(wk, r, lg, d_planes, poff); break;
        case 1: split_tile_grid<E, 1>(wk, r, lg, d_planes, poff); break;
        case 2: split_tile_grid<E, 2>(wk, r, lg, d_planes, poff); break;
        default: split_tile_grid<E, 3>(wk, r, lg, d_planes, poff); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- error-bounded fields (shafa_hipd_split_planes_grid_quant_dev, shafa_hipd_merge_planes_grid_quant_dev): the grid
// split over the CODES of float or double elements, code = rint(x (x) inv) as a signed integer of the element's width, taken
// unit by unit in registers as the units are loaded, the lane's own and every tap's alike: a code is a function of the element's
// own bits, so a tap's unit quantises to what the lane that owns it stores, and the bit pattern 0 in front of the block to the
// code 0.  Every operation is ONE IEEE operation in T, none contracted, the decoder's T(code) (x) step among them: the encoder
// judges the very value the decoder will make.
template <int E> struct FieldT { using F = float; using I = int; using U = u32; };
template <> struct FieldT<8> { using F = double; using I = long long; using U = u64; };
template <> struct FieldT<2> { using F = float; using I = short; using U = u16; };     // the patch pass alone: a record's 16 bits

// a block's step, 1 / step and bound as T (uniform)
template <int E> struct FieldQ {
    typename FieldT<E>::F step, inv, bound;
};

template <int E>
__device__ __forceinline__ typename FieldT<E>::F field_bits(u64 v)
{
    using U = typename FieldT<E>::U;
    return __builtin_bit_cast(typename FieldT<E>::F, (U)v);
}

// element i of the unit in w
template <int E>
__device__ __forceinline__ typename FieldT<E>::U unit_elem(const u32 (&w)[4 * E], int i)
{
    if (E == 8) return (typename FieldT<E>::U)((u64)w[2 * i + 1] << 32 | w[2 * i]);
    return (typename FieldT<E>::U)w[i];
}

__device__ __forceinline__ float field_abs(float t) { return __builtin_fabsf(t); }
__device__ __forceinline__ double field_abs(double t) { return __builtin_fabs(t); }
__device__ __forceinline__ float field_rint(float t) { return __builtin_rintf(t); }
__device__ __forceinline__ double field_rint(double t) { return __builtin_rint(t); }

// the code of the element with the bits xb; `in`: the scaled value lies inside the code range (false for a NaN)
template <int E>
__device__ __forceinline__ typename FieldT<E>::I field_code(typename FieldT<E>::U xb, typename FieldT<E>::F inv, bool &in)
{
#pragma clang fp contract(off)
    using F = typename FieldT<E>::F;
    using I = typename FieldT<E>::I;
    const F t = __builtin_bit_cast(F, xb) * inv;
    in = field_abs(t) < (F)(E == 8 ? 0x1p62 : 0x1p30);
    return (I)(in ? field_rint(t) : (F)0);
}

// the value the decoder makes of a code
template <int E>
__device__ __forceinline__ typename FieldT<E>::F field_value(typename FieldT<E>::I code, typename FieldT<E>::F step)
{
#pragma clang fp contract(off)
    return (typename FieldT<E>::F)code * step;
}

// is x' = T(code) (x) step within the bound of x?  At 4 bytes the subtraction is in double, which holds it exactly; at 8 it is
// the rounded one
template <int E>
__device__ __forceinline__ bool field_good(typename FieldT<E>::U xb, typename FieldT<E>::I code, const FieldQ<E> &q)
{
#pragma clang fp contract(off)
    using F = typename FieldT<E>::F;
    const F x = __builtin_bit_cast(F, xb), xr = field_value<E>(code, q.step);
    if (E == 8) return __builtin_fabs((double)(x - xr)) <= (double)q.bound;
    return __builtin_fabs((double)x - (double)xr) <= (double)q.bound;
}

// the 16 elements of w -> their codes as unsigned integers, in place; bad(i, bits) for each of the first c that is not good
template <int E, class F>
__device__ __forceinline__ void quant_unit(u32 (&w)[4 * E], const FieldQ<E> &q, u32 c, F &&bad)
{
#pragma unroll
    for (int i = 0; i < PL_UNIT; ++i) {
        using U = typename FieldT<E>::U;
        bool in;
        const U xb = unit_elem<E>(w, i);
        const typename FieldT<E>::I code = field_code<E>(xb, q.inv, in);
        if ((u32)i < c && !(in && field_good<E>(xb, code, q))) bad(i, (u64)xb);
        if (E == 8) { w[2 * i] = (u32)(U)code; w[2 * i + 1] = (u32)((u64)(U)code >> 32); }
        else w[i] = (u32)(U)code;
    }
}

// a tap's unit: nothing is judged
template <int E>
__device__ __forceinline__ void quant_words(u32 (&w)[4 * E], const FieldQ<E> &q)
{
    quant_unit<E>(w, q, 0u, [](int, u64) {});
}

// where a block's outliers go: records of {position, bits}, `cap` of them at the most, *count the outliers found
struct FieldOutl {
    u64 *rec, cap;
    unsigned long long *count;
};

// what the quantising and the rounding split do with an element of the lane's OWN unit that is not good: it is recorded in a slot
// of the block's, taken with an atomic of the lane's own (outliers are rare) and written only where it lies inside the block's
// capacity
__device__ __forceinline__ void outl_record(const FieldOutl &o, u64 pos, u64 bits)
{
    const u64 slot = atomicAdd(o.count, 1ull);
    if (slot < o.cap) {
        gstore<u64>(o.rec + 2 * slot, pos);
        gstore<u64>(o.rec + 2 * slot + 1, bits);
    }
}

// the quantising split's tile: the lane's own unit quantised and judged, a tap's unit quantised, then the grid split's sink
template <int E, int Q>
__device__ __forceinline__ void split_tile_grid_quant(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS],
                                                      const FieldQ<E> &q, const FieldOutl &o, u8 *d_planes, const u64 *poff)
{
    grid_tile<E, Q>(
        wk, r, lg, [&](u32 (&w)[4 * E], u64 e0, u32 c) { quant_unit<E>(w, q, c, [&](int i, u64 xb) { outl_record(o, e0 + (u64)i, xb); }); },
        [&](u32 (&wb)[4 * E]) { quant_words<E>(wb, q); },
        [&](u32 (&w)[4 * E], u64 e0, u32) {
            zz_fold<E, 4 * E>(w);
            split_store<E>(w, wk.n, e0, d_planes, poff);
        });
}

// d_lag: planes_grid_split's rows of clamped lags and behind them five rows of nblk: the bits of step, 1 / step and bound as T,
// the block's first record in d_outl and its capacity in records.  d_outl_n has been zeroed on the stream.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_quant_split(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                      const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                      int nblk, const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                                      const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                                      int *__restrict__ err, u32 n_tiles, u32 per_wg,
                                                                      u64 *__restrict__ d_outl, u64 *__restrict__ d_outl_n)
{
    const u64 *qp = d_lag + (u64)SHAFA_PLANES_GRID_LAGS * nblk;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const FieldQ<E> q = {field_bits<E>(qp[wk.b]), field_bits<E>(qp[(u64)nblk + wk.b]), field_bits<E>(qp[2ull * nblk + wk.b])};
        const FieldOutl o = {d_outl + 2 * qp[3ull * nblk + wk.b], qp[4ull * nblk + wk.b], (unsigned long long *)d_outl_n + wk.b};
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: split_tile_grid_quant<E, 0>(wk, r, lg, q, o, d_planes, poff); break;
        case 1: split_tile_grid_quant<E, 1>(wk, r, lg, q, o, d_planes, poff); break;
        case 2: split_tile_grid_quant<E, 2>(wk, r, lg, q, o, d_planes, poff); break;
        default: split_tile_grid_quant<E, 3>(wk, r, lg, q, o, d_planes, poff); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- point-wise relative bounds (shafa_hipd_split_planes_grid_round_dev and its two companions): the grid split over
// the CODES of bfloat16, float16, float or double elements whose mantissa is rounded to `keep` of its `mant` bits, half to even,
// the carry free to enter the exponent.  All of it is unsigned integer arithmetic of the element's width W = 8 E on the element's
// own bits (include/shafa_hip.h: "Point-wise relative bounds"), so a tap's unit rounds to what the lane that owns it stores and the
// bit pattern 0 in front of the block to the code 0.  At E = 2 an element is taken out of its word, rounded in 32 bits and put
// back masked to 16: no carry passes from one half of a word into the other.
template <int E> struct RoundT { using U = u32; };
template <> struct RoundT<8> { using U = u64; };

// a block's rounding (uniform): d = mant - keep dropped bits; half = 2^(d - 1) - 1 and tie = 1, both 0 at d = 0; inf the bits of
// +Inf, min those of the smallest normal
template <int E> struct RoundQ {
    typename RoundT<E>::U half, tie, inf, min;
    u32 d;
    __device__ __forceinline__ RoundQ(u64 row)       // the block's row: d in the low byte, mant in the next
    {
        using U = typename RoundT<E>::U;
        const u32 mant = (u32)(row >> 8) & 0xFFu;
        d = (u32)row & 0xFFu;
        half = d ? (U)(((U)1 << (d - 1)) - 1) : (U)0;
        tie = d ? 1 : 0;
        inf = (U)((((U)1 << (8 * E - 1 - mant)) - 1) << mant);
        min = (U)1 << mant;
    }
};

// the code of the element with the bits x (E = 2: in the low 16 bits, and so is the code), and whether it is good
template <int E>
__device__ __forceinline__ typename RoundT<E>::U round_code(typename RoundT<E>::U x, const RoundQ<E> &q, bool &good)
{
    using U = typename RoundT<E>::U;
    constexpr u32 W = 8 * E;
    constexpr U MAG = (U)(((U)1 << (W - 1)) - 1);
    const U m = x & MAG;
    const bool special = m >= q.inf;                 // Inf and NaN: truncated, never carried
    const U r = special ? (U)(m >> q.d) : (U)((U)(m + q.half + ((m >> q.d) & q.tie)) >> q.d);
    const U back = (U)(r << q.d) & MAG;              // what the merge makes of the code
    good = (special || m < q.min) ? back == m : back < q.inf;
    const U code = (x >> (W - 1)) & 1 ? (U)(0 - r) : r;
    return E == 2 ? (U)(code & 0xFFFFu) : code;
}

// the bits the merge makes of ANY code
template <int E>
__device__ __forceinline__ typename RoundT<E>::U round_value(typename RoundT<E>::U code, u32 d)
{
    using U = typename RoundT<E>::U;
    constexpr u32 W = 8 * E;
    constexpr U MAG = (U)(((U)1 << (W - 1)) - 1);
    const U neg = (code >> (W - 1)) & 1;
    const U a = neg ? (U)(0 - code) : code;
    return (U)(neg << (W - 1)) | ((U)(a << d) & MAG);
}

// the 16 elements of w -> their codes as unsigned integers, in place; bad(i, bits) for each of the first c that is not good
template <int E, class F>
__device__ __forceinline__ void round_unit(u32 (&w)[4 * E], const RoundQ<E> &q, u32 c, F &&bad)
{
#pragma unroll
    for (int i = 0; i < PL_UNIT; ++i) {
        using U = typename RoundT<E>::U;
        const U xb = E == 8 ? (U)((u64)w[(2 * i + 1) % (4 * E)] << 32 | w[(2 * i) % (4 * E)])
                   : E == 4 ? (U)w[i % (4 * E)] : (U)((w[(i >> 1) % (4 * E)] >> (16 * (i & 1))) & 0xFFFFu);
        bool good;
        const U code = round_code<E>(xb, q, good);
        if ((u32)i < c && !good) bad(i, (u64)xb);
        if (E == 8) { w[(2 * i) % (4 * E)] = (u32)code; w[(2 * i + 1) % (4 * E)] = (u32)((u64)code >> 32); }
        else if (E == 4) w[i % (4 * E)] = (u32)code;
        else w[(i >> 1) % (4 * E)] = (i & 1) ? (w[(i >> 1) % (4 * E)] & 0xFFFFu) | (u32)code << 16
                                             : (w[(i >> 1) % (4 * E)] & 0xFFFF0000u) | (u32)code;
    }
}

// a tap's unit: nothing is judged
template <int E>
__device__ __forceinline__ void round_words(u32 (&w)[4 * E], const RoundQ<E> &q)
{
    round_unit<E>(w, q, 0u, [](int, u64) {});
}

// the rounding split's tile: split_tile_grid_quant with the rounding for the quantiser
template <int E, int Q>
__device__ __forceinline__ void split_tile_grid_round(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS],
                                                      const RoundQ<E> &q, const FieldOutl &o, u8 *d_planes, const u64 *poff)
{
    grid_tile<E, Q>(
        wk, r, lg, [&](u32 (&w)[4 * E], u64 e0, u32 c) { round_unit<E>(w, q, c, [&](int i, u64 xb) { outl_record(o, e0 + (u64)i, xb); }); },
        [&](u32 (&wb)[4 * E]) { round_words<E>(wb, q); },
        [&](u32 (&w)[4 * E], u64 e0, u32) {
            zz_fold<E, 4 * E>(w);
            split_store<E>(w, wk.n, e0, d_planes, poff);
        });
}

// d_lag: planes_grid_split's rows of clamped lags and behind them planes_grid_quant_split's five rows of nblk, the first d | mant
// << 8 and the next two unused: then the block's first record in d_outl and its capacity in records.  d_outl_n has been zeroed on
// the stream.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_round_split(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                      const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                      int nblk, const u64 *__restrict__ d_n, u8 *__restrict__ d_planes,
                                                                      const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                                      int *__restrict__ err, u32 n_tiles, u32 per_wg,
                                                                      u64 *__restrict__ d_outl, u64 *__restrict__ d_outl_n)
{
    const u64 *qp = d_lag + (u64)SHAFA_PLANES_GRID_LAGS * nblk;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u64 *poff = d_poff + (u64)wk.b * E;
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const RoundQ<E> q(qp[wk.b]);
        const FieldOutl o = {d_outl + 2 * qp[3ull * nblk + wk.b], qp[4ull * nblk + wk.b], (unsigned long long *)d_outl_n + wk.b};
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: split_tile_grid_round<E, 0>(wk, r, lg, q, o, d_planes, poff); break;
        case 1: split_tile_grid_round<E, 1>(wk, r, lg, q, o, d_planes, poff); break;
        case 2: split_tile_grid_round<E, 2>(wk, r, lg, q, o, d_planes, poff); break;
        default: split_tile_grid_round<E, 3>(wk, r, lg, q, o, d_planes, poff); break;
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- the histograms of the grid split's planes without the planes (shafa_hipd_hist_planes_grid_dev): the split's
// grid_tile, and where split_store would write one word of each plane, the word's bytes are counted into a
// replicated LDS histogram per plane (hist.hip's layout: bin s of replica r at s REP + r, a lane's replica from its number).  The
// high planes of good differences are one byte nearly everywhere; the replicas alone carry that (folding a lane's 16 equal bytes
// into one atomic measured 1 % SLOWER: DESIGN 7.29).  Only the c = min(16, n - e0) elements in front of the block's end are
// counted: the unit's bytes behind them are whatever lies behind the region.  A workgroup walks a run of SHAFA_PLANES_HIST_RUN
// consecutive tiles and adds its non-zero bins to the block's counts, with 64-bit global atomics, when the walk enters another
// block and at its end (flush: rle_encode_hist.hip's).  A bin of a replica takes at most RUN x 8192 elements between two
// flushes, so 32-bit LDS counters hold.
constexpr u32 GH_RUN = SHAFA_PLANES_HIST_RUN;
// replicas: hist.hip's 32 at E = 1; 8 at E = 2 and 4, the fastest measured (16 and 32 KiB of LDS: DESIGN 7.29); 4 at E = 8, where 8
// would be 64 KiB and two workgroups a CU
template <int E> constexpr u32 gh_rep() { return E == 1 ? 32u : E == 8 ? 4u : 8u; }
static_assert((u64)GH_RUN * TP_TILE < (1ull << 32), "a run's elements fit one 32-bit bin");

template <int E>
__device__ __forceinline__ void hist_count(const u32 (&w)[4 * E], u32 c, u32 *h)
{
    constexpr u32 REP = gh_rep<E>();
    const u32 rep = threadIdx.x & (REP - 1u);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const u32 o[4] = {split_dword<E>(w, j, 0), split_dword<E>(w, j, 1), split_dword<E>(w, j, 2), split_dword<E>(w, j, 3)};
        u32 *hj = h + (u32)j * 256u * REP + rep;
        if (c == PL_UNIT) {
#pragma unroll
            for (int k = 0; k < PL_UNIT; ++k) atomicAdd(hj + ((o[k >> 2] >> (8 * (k & 3))) & 0xFFu) * REP, 1u);
        } else {
#pragma unroll
            for (int k = 0; k < PL_UNIT; ++k)
                if ((u32)k < c) atomicAdd(hj + ((o[k >> 2] >> (8 * (k & 3))) & 0xFFu) * REP, 1u);
        }
    }
}

// the three histograms' tiles: the splits' with hist_count for split_store and, for the record, a count in the lane's outl; the
// fold is left out for a block of plain planes (fold, uniform)
template <int E, int Q>
__device__ __forceinline__ void hist_tile_grid(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS], bool fold, u32 *h)
{
    grid_tile<E, Q>(wk, r, lg, [](u32 (&)[4 * E], u64, u32) {}, [](u32 (&)[4 * E]) {}, [&](u32 (&w)[4 * E], u64, u32 c) {
        if (fold) zz_fold<E, 4 * E>(w);              // (uniform)
        hist_count<E>(w, c, h);
    });
}

// planes_grid_quant_hist keeps a walk and a body of its own, the text they had before grid_tile and grid_hist: through the shared
// ones its float32 (1, 4096) and float64 (1,) legs measured 0.1 to 0.6 % over the unchanged kernel's in two alternated runs
// (LABNOTES, "one grid tile walk").  A change to grid_tile or to grid_hist has to be made here as well.
template <int E, int Q>
__device__ __forceinline__ void hist_tile_grid_quant(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS],
                                                     const FieldQ<E> &q, u32 *h, u32 &outl)
{
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u64 e0 = wk.pos0 + (u64)u * PL_PASS + (u64)threadIdx.x * PL_UNIT;
        if (e0 >= wk.n) continue;
        u32 w[4 * E];
        {
            uint4 a[E + 1];
            load_words<E, true>(wk.in, wk.n * E, e0 * E, 4u * Q + r, a);
            shift_into<E, Q, false>(a, r, w);
        }
        const u32 c = wk.n - e0 >= PL_UNIT ? (u32)PL_UNIT : (u32)(wk.n - e0);
#pragma unroll
        for (int i = 0; i < PL_UNIT; ++i) {          // quant_unit with a count for the record
            using U = typename FieldT<E>::U;
            bool in;
            const U xb = unit_elem<E>(w, i);
            const typename FieldT<E>::I code = field_code<E>(xb, q.inv, in);
            if ((u32)i < c && !(in && field_good<E>(xb, code, q))) ++outl;
            if (E == 8) { w[2 * i] = (u32)(U)code; w[2 * i + 1] = (u32)((u64)(U)code >> 32); }
            else w[i] = (u32)(U)code;
        }
#pragma nounroll
        for (u32 sub = 1; sub < 1u << SHAFA_PLANES_GRID_LAGS; ++sub) {          // (uniform)
            u64 dist = 0;
            bool used = true;
#pragma unroll
            for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k)
                if (sub >> k & 1u) {
                    used = used && lg[k] != 0;
                    dist += lg[k];
                }
            if (!used) continue;                     // (uniform)
            if (e0 + PL_UNIT > dist) {
                u32 wb[4 * E];
                lag_base<E>(wk.in, wk.n, dist, e0, wb);
                quant_words<E>(wb, q);               // the zeros in front of the block stay zeros
                if (__builtin_popcount(sub) & 1) sub_words<E>(w, wb);           // (uniform)
                else add_words<E>(w, wb);
            }
        }
        zz_fold<E, 4 * E>(w);
        hist_count<E>(w, c, h);
    }
}

template <int E, int Q>
__device__ __forceinline__ void hist_tile_grid_round(const TpWalk &wk, u32 r, const u64 (&lg)[SHAFA_PLANES_GRID_LAGS],
                                                     const RoundQ<E> &q, u32 *h, u32 &outl)
{
    grid_tile<E, Q>(
        wk, r, lg, [&](u32 (&w)[4 * E], u64, u32 c) { round_unit<E>(w, q, c, [&](int, u64) { ++outl; }); },
        [&](u32 (&wb)[4 * E]) { round_words<E>(wb, q); },
        [&](u32 (&w)[4 * E], u64, u32 c) {
            zz_fold<E, 4 * E>(w);
            hist_count<E>(w, c, h);
        });
}

// the body of the histogram kernels (planes_grid_quant_hist keeps a copy of its own): the bins, the walk in runs of GH_RUN tiles and the flushes.  tile(wk, h, outl) makes
// the block's parameters from its rows and walks the tile wk has entered, counting into h.  OUTL: the kernel counts outliers as
// well.  A lane adds its own to the register outl (a run is at most GH_RUN x 32 elements a lane), and flush adds the waves' sums
// to the block's d_outl_n, one 64-bit atomic a wave that found any: a tensor of noise at a tiny bound, where every element is an
// outlier, costs 4 atomics a run so and not 65536.
template <int E, bool OUTL, class Tile>
__device__ __forceinline__ void grid_hist(const u8 *d_el, const u64 *off, const u64 *cap, const u32 *tbase, int nblk, const u64 *d_n,
                                          int *err, u32 n_tiles, u64 *d_freq, u64 *d_outl_n, Tile &&tile)
{
    constexpr u32 REP = gh_rep<E>(), GH_BINS = 256u * E * REP;
    __shared__ u32 h[GH_BINS];                       // bin s of replica r of plane j at (j 256 + s) REP + r
    const u32 tid = threadIdx.x;
    u32 outl = 0;                                    // the lane's outliers of block cur_b since the last flush
    // the workgroup's bins -> block b's counts; every thread sums and clears the replicas of bin tid of each plane (rotated); the
    // lane's counter is cleared with the bins
    auto flush = [&](int b) {
        lds_barrier();
#pragma unroll
        for (int j = 0; j < E; ++j) {
            u32 c = 0;
#pragma unroll
            for (u32 q = 0; q < REP; ++q) {
                u32 *p = &h[((u32)j * 256u + tid) * REP + ((q + tid) & (REP - 1u))];
                c += *p;
                *p = 0;
            }
            if (c) atomicAdd((unsigned long long *)(d_freq + ((size_t)b * E + j) * 256 + tid), (unsigned long long)c);
        }
        if constexpr (OUTL) {
            const u32 wsum = wave_reduce_add<u32>(outl);
            if (wsum && lane_id() == 0) atomicAdd((unsigned long long *)d_outl_n + b, (unsigned long long)wsum);
            outl = 0;
        }
        lds_barrier();
    };
    for (u32 i = tid; i < GH_BINS; i += TP_THREADS) h[i] = 0;
    lds_barrier();
    int cur_b = -1;                                  // the block whose counts the bins and the counter hold
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, GH_RUN); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur_b) {                         // (uniform)
            if (cur_b >= 0) flush(cur_b);
            cur_b = wk.b;
        }
        tile(wk, h, outl);
    }
    if (cur_b >= 0) flush(cur_b);
    tp_size_errors(cap, d_n, nblk, err);
}

// d_lag: planes_grid_split's rows of clamped lags and behind them a row of flags, 0 for a block of plain planes (a row of zeros
// from the caller), else 1: the clamped lags alone do not tell the two apart
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_hist(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                               const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                               const u64 *__restrict__ d_n, const u64 *__restrict__ d_lag,
                                                               int *__restrict__ err, u32 n_tiles, u64 *__restrict__ d_freq)
{
    grid_hist<E, false>(d_el, off, cap, tbase, nblk, d_n, err, n_tiles, d_freq, nullptr, [&](const TpWalk &wk, u32 *h, u32 &) {
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const bool fold = d_lag[(u64)SHAFA_PLANES_GRID_LAGS * nblk + wk.b] != 0;
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: hist_tile_grid<E, 0>(wk, r, lg, fold, h); break;
        case 1: hist_tile_grid<E, 1>(wk, r, lg, fold, h); break;
        case 2: hist_tile_grid<E, 2>(wk, r, lg, fold, h); break;
        default: hist_tile_grid<E, 3>(wk, r, lg, fold, h); break;
        }
    });
}

// ---- the histograms of the QUANTISING split's planes without the planes (shafa_hipd_hist_planes_grid_quant_dev):
// planes_grid_hist over the codes, with the quantising split's callables for the lane's own unit and a tap's, the fold always,
// and the outliers COUNTED where the split records them (grid_hist's outl).
// d_lag: planes_grid_split's rows of clamped lags and behind them three rows of nblk: the bits of step, 1 / step and bound as T.
// d_freq and d_outl_n have been zeroed on the stream.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_quant_hist(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                     const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                     int nblk, const u64 *__restrict__ d_n,
                                                                     const u64 *__restrict__ d_lag, int *__restrict__ err,
                                                                     u32 n_tiles, u64 *__restrict__ d_freq,
                                                                     u64 *__restrict__ d_outl_n)
{
    constexpr u32 REP = gh_rep<E>(), GH_BINS = 256u * E * REP;
    __shared__ u32 h[GH_BINS];                       // bin s of replica r of plane j at (j 256 + s) REP + r
    const u32 tid = threadIdx.x;
    u32 outl = 0;                                    // the lane's outliers of block cur_b since the last flush
    // grid_hist's flush
    auto flush = [&](int b) {
        lds_barrier();
#pragma unroll
        for (int j = 0; j < E; ++j) {
            u32 c = 0;
#pragma unroll
            for (u32 q = 0; q < REP; ++q) {
                u32 *p = &h[((u32)j * 256u + tid) * REP + ((q + tid) & (REP - 1u))];
                c += *p;
                *p = 0;
            }
            if (c) atomicAdd((unsigned long long *)(d_freq + ((size_t)b * E + j) * 256 + tid), (unsigned long long)c);
        }
        const u32 wsum = wave_reduce_add<u32>(outl);
        if (wsum && lane_id() == 0) atomicAdd((unsigned long long *)d_outl_n + b, (unsigned long long)wsum);
        outl = 0;
        lds_barrier();
    };
    for (u32 i = tid; i < GH_BINS; i += TP_THREADS) h[i] = 0;
    lds_barrier();
    const u64 *qp = d_lag + (u64)SHAFA_PLANES_GRID_LAGS * nblk;
    int cur_b = -1;                                  // the block whose counts the bins and the counters hold
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, GH_RUN); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        if (wk.b != cur_b) {                         // (uniform)
            if (cur_b >= 0) flush(cur_b);
            cur_b = wk.b;
        }
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const FieldQ<E> q = {field_bits<E>(qp[wk.b]), field_bits<E>(qp[(u64)nblk + wk.b]), field_bits<E>(qp[2ull * nblk + wk.b])};
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: hist_tile_grid_quant<E, 0>(wk, r, lg, q, h, outl); break;
        case 1: hist_tile_grid_quant<E, 1>(wk, r, lg, q, h, outl); break;
        case 2: hist_tile_grid_quant<E, 2>(wk, r, lg, q, h, outl); break;
        default: hist_tile_grid_quant<E, 3>(wk, r, lg, q, h, outl); break;
        }
    }
    if (cur_b >= 0) flush(cur_b);
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- the histograms of the ROUNDING split's planes without the planes (shafa_hipd_hist_planes_grid_round_dev):
// planes_grid_quant_hist with the rounding for the quantiser.
// d_lag: planes_grid_split's rows of clamped lags and behind them one row of nblk: d | mant << 8.  d_freq and d_outl_n have been
// zeroed on the stream.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_grid_round_hist(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                     const u64 *__restrict__ cap, const u32 *__restrict__ tbase,
                                                                     int nblk, const u64 *__restrict__ d_n,
                                                                     const u64 *__restrict__ d_lag, int *__restrict__ err,
                                                                     u32 n_tiles, u64 *__restrict__ d_freq,
                                                                     u64 *__restrict__ d_outl_n)
{
    const u64 *qp = d_lag + (u64)SHAFA_PLANES_GRID_LAGS * nblk;
    grid_hist<E, true>(d_el, off, cap, tbase, nblk, d_n, err, n_tiles, d_freq, d_outl_n, [&](const TpWalk &wk, u32 *h, u32 &outl) {
        u64 lg[SHAFA_PLANES_GRID_LAGS];
#pragma unroll
        for (int k = 0; k < SHAFA_PLANES_GRID_LAGS; ++k) lg[k] = d_lag[(u64)k * nblk + wk.b];
        const RoundQ<E> q(qp[wk.b]);
        const u32 sh = (u32)((uintptr_t)wk.in & 15u), r = sh & 3u;
        switch (sh >> 2) {                           // uniform
        case 0: hist_tile_grid_round<E, 0>(wk, r, lg, q, h, outl); break;
        case 1: hist_tile_grid_round<E, 1>(wk, r, lg, q, h, outl); break;
        case 2: hist_tile_grid_round<E, 2>(wk, r, lg, q, h, outl); break;
        default: hist_tile_grid_round<E, 3>(wk, r, lg, q, h, outl); break;
        }
    });
}

// ---- error statistics (shafa_hipd_error_dev, shafa_hipd_error_quant_dev, shafa_hipd_error_round_dev): what a bound
// costs.  x is the original element and y the element it comes back as: the element of a second tensor (ERR_PAIR), or what the
// quantising (ERR_QUANT) or the rounding (ERR_ROUND) merge would give back, made in registers from x with the split's own
// functions — x' where the element is good, x's own bits where it is an outlier.  The walk is grid_tile's without taps,
// bins or LDS histograms: a lane loads its units of 16 elements and folds them, by index, into an ErrAgg.  Every sum, product and
// comparison is one IEEE double operation, none contracted, and the order is fixed: the lane's elements by index, err_wave_reduce's
// tree across the wave, the four waves in order, one partial of SHAFA_ERR_WORDS words a tile; planes_error_blocks folds a block's
// partials in ascending tile order the same way.  No atomics: a block's record is a function of its elements, its count and its
// parameters alone.
constexpr u32 ERR_WORDS = SHAFA_ERR_WORDS;
constexpr u64 ERR_NONE = ~0ull;

// the statistics of a piece of a block: words 1 .. 11 of the record (include/shafa_hip.h: "Error statistics")
struct ErrAgg {
    u64 fin, oth, diff, outl, over;
    double se2, sx2, emax;
    u64 arg;
    double xmin, xmax;
};

__device__ __forceinline__ ErrAgg err_identity()
{
    return {0, 0, 0, 0, 0, 0.0, 0.0, 0.0, ERR_NONE, __builtin_inf(), -__builtin_inf()};
}

// a's piece, then b's.  The largest error's position is the smallest one that holds it whatever the order of the pieces.
__device__ __forceinline__ ErrAgg err_then(const ErrAgg &a, const ErrAgg &b)
{
#pragma clang fp contract(off)
    ErrAgg r;
    r.fin = a.fin + b.fin; r.oth = a.oth + b.oth; r.diff = a.diff + b.diff; r.outl = a.outl + b.outl; r.over = a.over + b.over;
    r.se2 = a.se2 + b.se2;
    r.sx2 = a.sx2 + b.sx2;
    const bool tb = b.emax > a.emax || (b.emax == a.emax && b.arg < a.arg);
    r.emax = tb ? b.emax : a.emax;
    r.arg = tb ? b.arg : a.arg;
    r.xmin = b.xmin < a.xmin ? b.xmin : a.xmin;
    r.xmax = b.xmax > a.xmax ? b.xmax : a.xmax;
    return r;
}

__device__ __forceinline__ ErrAgg err_from_lane(const ErrAgg &a, int d)
{
    ErrAgg o;
    o.fin = __shfl_down((unsigned long long)a.fin, d, 64); o.oth = __shfl_down((unsigned long long)a.oth, d, 64);
    o.diff = __shfl_down((unsigned long long)a.diff, d, 64); o.outl = __shfl_down((unsigned long long)a.outl, d, 64);
    o.over = __shfl_down((unsigned long long)a.over, d, 64);
    o.se2 = __shfl_down(a.se2, d, 64); o.sx2 = __shfl_down(a.sx2, d, 64); o.emax = __shfl_down(a.emax, d, 64);
    o.arg = __shfl_down((unsigned long long)a.arg, d, 64);
    o.xmin = __shfl_down(a.xmin, d, 64); o.xmax = __shfl_down(a.xmax, d, 64);
    return o;
}

// tp_wave_reduce's tree: after the step of distance d lane l holds lanes [l, l + 2 d); lane 0 ends with the wave's
__device__ __forceinline__ ErrAgg err_wave_reduce(ErrAgg a)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const ErrAgg o = err_from_lane(a, d);
        if (lane + d < 64) a = err_then(a, o);
    }
    return a;
}

// a piece's words 1 .. 11 at p (word 0 is the record's n, 0 in a partial)
__device__ __forceinline__ void err_put(u64 *p, const ErrAgg &a)
{
    p[1] = a.fin; p[2] = a.oth; p[3] = a.diff; p[4] = a.outl; p[5] = a.over;
    p[6] = __builtin_bit_cast(u64, a.se2); p[7] = __builtin_bit_cast(u64, a.sx2); p[8] = __builtin_bit_cast(u64, a.emax);
    p[9] = a.arg;
    p[10] = __builtin_bit_cast(u64, a.xmin); p[11] = __builtin_bit_cast(u64, a.xmax);
}

__device__ __forceinline__ ErrAgg err_get(const u64 *p)
{
    return {p[1], p[2], p[3], p[4], p[5], __builtin_bit_cast(double, p[6]), __builtin_bit_cast(double, p[7]),
            __builtin_bit_cast(double, p[8]), p[9], __builtin_bit_cast(double, p[10]), __builtin_bit_cast(double, p[11])};
}

// the four waves' results in LDS, in order
__device__ __forceinline__ ErrAgg err_waves(const u64 *slot)
{
    ErrAgg a = err_get(slot);
#pragma unroll
    for (int q = 1; q < TP_THREADS / 64; ++q) a = err_then(a, err_get(slot + (u32)q * ERR_WORDS));
    return a;
}

// D(.): the element's value as a double, exact.  At 2 bytes it is taken from the bits: bfloat16 is the top half of a float,
// float16 is put together from its fields (bf16: the block's format, uniform).
template <int E>
__device__ __forceinline__ double err_value(typename RoundT<E>::U bits, bool bf16)
{
#pragma clang fp contract(off)
    if (E == 8) return __builtin_bit_cast(double, (u64)bits);
    if (E == 4) return (double)__builtin_bit_cast(float, (u32)bits);
    if (bf16) return (double)__builtin_bit_cast(float, (u32)bits << 16);
    const u32 b = (u32)bits, ex = (b >> 10) & 31u, m = b & 0x3FFu;
    const u64 s = (u64)((b >> 15) & 1u) << 63;
    u64 d;
    if (ex == 31u) d = 0x7FFull << 52 | (u64)m << 42;                          // Inf, NaN
    else if (ex) d = (u64)(ex + 1008u) << 52 | (u64)m << 42;                   // normal: the exponent rebiased from 15 to 1023
    else d = __builtin_bit_cast(u64, (double)(int)m * 0x1p-24);                // denormal or zero: m 2^-24
    return __builtin_bit_cast(double, s | d);
}

// element i of the unit in w, E = 2 included (unit_elem there has the code's width)
template <int E>
__device__ __forceinline__ typename RoundT<E>::U err_elem(const u32 (&w)[4 * E], int i)
{
    if constexpr (E == 2) return (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    else return (typename RoundT<E>::U)unit_elem<E>(w, i);
}

// a block's parameters (uniform), from its three words of the launch's rows: ERR_PAIR mant, the bits of abs and of rel;
// ERR_QUANT the bits of step, 1 / step and bound as T; ERR_ROUND d | mant << 8
template <int E, int SRC> struct ErrQ;
template <int E> struct ErrQ<E, ERR_PAIR> {
    bool bf16;
    double abs, rel;
    __device__ __forceinline__ ErrQ(u64 q0, u64 q1, u64 q2)
        : bf16(q0 == 7), abs(__builtin_bit_cast(double, q1)), rel(__builtin_bit_cast(double, q2)) {}
};
template <int E> struct ErrQ<E, ERR_QUANT> {
    static constexpr bool bf16 = false;
    FieldQ<E> q;
    __device__ __forceinline__ ErrQ(u64 q0, u64 q1, u64 q2) : q{field_bits<E>(q0), field_bits<E>(q1), field_bits<E>(q2)} {}
};
template <int E> struct ErrQ<E, ERR_ROUND> {
    bool bf16;
    RoundQ<E> q;
    __device__ __forceinline__ ErrQ(u64 q0, u64, u64) : bf16(((q0 >> 8) & 0xFFu) == 7), q(q0) {}
};

// the bits element xb comes back as under the block's rule, and whether it is good (an outlier comes back bit for bit)
template <int E>
__device__ __forceinline__ typename RoundT<E>::U err_back(typename RoundT<E>::U xb, const ErrQ<E, ERR_QUANT> &p, bool &good)
{
    using U = typename FieldT<E>::U;
    bool in;
    const typename FieldT<E>::I code = field_code<E>((U)xb, p.q.inv, in);
    good = in && field_good<E>((U)xb, code, p.q);
    return good ? (typename RoundT<E>::U)__builtin_bit_cast(U, field_value<E>(code, p.q.step)) : xb;
}

template <int E>
__device__ __forceinline__ typename RoundT<E>::U err_back(typename RoundT<E>::U xb, const ErrQ<E, ERR_ROUND> &p, bool &good)
{
    const typename RoundT<E>::U code = round_code<E>(xb, p.q, good);
    return good ? round_value<E>(code, p.q.d) : xb;
}

// one tile of one lane: its PL_UNITS units of 16 elements, by index.  x is read at xs (xs mod 16 = 4 Q + r, any multiple of E);
// ERR_PAIR: y at wk.in, a multiple of 16.  wk.n elements in both.
template <int E, int SRC, int Q>
__device__ __forceinline__ ErrAgg err_tile(const TpWalk &wk, const u8 *xs, u32 r, const ErrQ<E, SRC> &p)
{
#pragma clang fp contract(off)
    using U = typename RoundT<E>::U;
    constexpr u32 NONE = ~0u;
    const double inf = __builtin_inf();
    u32 fin = 0, oth = 0, diff = 0, outl = 0, over = 0, arg = NONE;             // arg: the element's number within the tile
    double se2 = 0.0, sx2 = 0.0, emax = 0.0, xmin = inf, xmax = -inf;
#pragma nounroll
    for (int u = 0; u < PL_UNITS; ++u) {
        const u32 rel0 = (u32)u * PL_PASS + threadIdx.x * PL_UNIT;
        const u64 e0 = wk.pos0 + rel0;
        if (e0 >= wk.n) continue;
        u32 wx[4 * E], wy[SRC == ERR_PAIR ? 4 * E : 1];
        {
            uint4 a[E + 1];
            load_words<E, true>(xs, wk.n * E, e0 * E, 4u * Q + r, a);
            shift_into<E, Q, false>(a, r, wx);
        }
        if constexpr (SRC == ERR_PAIR) {
            uint4 a[E + 1];
            load_words<E, true>(wk.in, wk.n * E, e0 * E, 0u, a);
            shift_into<E, 0, false>(a, 0u, wy);
        }
        const u32 c = wk.n - e0 >= PL_UNIT ? (u32)PL_UNIT : (u32)(wk.n - e0);
#pragma unroll
        for (int i = 0; i < PL_UNIT; ++i) {
            if ((u32)i >= c) continue;
            const U xb = err_elem<E>(wx, i);
            U yb;
            if constexpr (SRC == ERR_PAIR) yb = err_elem<E>(wy, i);
            else {
                bool good;
                yb = err_back<E>(xb, p, good);
                if (!good) ++outl;
            }
            const double dx = err_value<E>(xb, p.bf16), dy = err_value<E>(yb, p.bf16);
            if (__builtin_fabs(dx) < inf && __builtin_fabs(dy) < inf) {
                const double e = __builtin_fabs(dx - dy);
                ++fin;
                se2 = se2 + e * e;
                sx2 = sx2 + dx * dx;
                if (e > emax || arg == NONE) { emax = e; arg = rel0 + (u32)i; }
                xmin = dx < xmin ? dx : xmin;
                xmax = dx > xmax ? dx : xmax;
                if constexpr (SRC == ERR_PAIR)
                    if (e > p.abs + p.rel * __builtin_fabs(dx)) ++over;
            } else {
                ++oth;
                if (yb != xb) ++diff;
            }
        }
    }
    return {fin, oth, diff, outl, over, se2, sx2, emax, arg == NONE ? ERR_NONE : wk.pos0 + arg, xmin, xmax};
}

// q: three rows of nblk words, ErrQ's.  ERR_PAIR: d_el is side a (y) and block b's x lies at d_ref + ref_off[b]; else d_el is x.
// part: ERR_WORDS words a tile of the capacities; the tiles below a block's d_n are written.
template <int E, int SRC>
__global__ __launch_bounds__(TP_THREADS) void planes_error_tiles(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                 const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                                 const u64 *__restrict__ d_n, const u8 *__restrict__ d_ref,
                                                                 const u64 *__restrict__ ref_off, const u64 *__restrict__ q,
                                                                 u64 *__restrict__ part, u32 n_tiles, u32 per_wg)
{
    __shared__ u64 wres[2][TP_THREADS / 64][ERR_WORDS];     // the waves' results; the halves alternate: one barrier a tile
    u32 turn = 0;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const ErrQ<E, SRC> p(q[wk.b], q[(u64)nblk + wk.b], q[2ull * nblk + wk.b]);
        const u8 *xs = SRC == ERR_PAIR ? d_ref + ref_off[wk.b] : wk.in;
        const u32 sh = (u32)((uintptr_t)xs & 15u), r = sh & 3u;
        ErrAgg a;
        switch (sh >> 2) {                           // uniform
        case 0: a = err_tile<E, SRC, 0>(wk, xs, r, p); break;
        case 1: a = err_tile<E, SRC, 1>(wk, xs, r, p); break;
        case 2: a = err_tile<E, SRC, 2>(wk, xs, r, p); break;
        default: a = err_tile<E, SRC, 3>(wk, xs, r, p); break;
        }
        a = err_wave_reduce(a);
        u64 *slot = &wres[turn & 1u][0][0];
        ++turn;
        if (lane_id() == 0) err_put(slot + (u32)wave_id() * ERR_WORDS, a);
        lds_barrier();
        if (threadIdx.x == 0) {
            u64 *dst = part + (u64)wk.t * ERR_WORDS;
            const ErrAgg t = err_waves(slot);
            u64 v[ERR_WORDS];
            v[0] = 0;
            err_put(v, t);
#pragma unroll
            for (u32 i = 0; i < ERR_WORDS; i += 2) gstore<uint4>(dst + i, make_uint4((u32)v[i], (u32)(v[i] >> 32), (u32)v[i + 1], (u32)(v[i + 1] >> 32)));
        }
    }
}

// one workgroup a block (grid-stride): a thread folds a run of consecutive partials in ascending tile order, then the same tree.
// d_n[b] > cap[b]: SHAFA_OUTSIDE_MODULE and a record of zeros.
__global__ __launch_bounds__(TP_THREADS) void planes_error_blocks(const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                                  const u64 *__restrict__ d_n, const u64 *__restrict__ part,
                                                                  u64 *__restrict__ d_stat, int *__restrict__ err)
{
    __shared__ u64 wres[TP_THREADS / 64][ERR_WORDS];
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
        const u64 n = d_n[b];
        u64 *rec = d_stat + (u64)b * ERR_WORDS;
        if (n > cap[b]) {                            // (uniform) past the block's region
            if (tid < (int)ERR_WORDS) gstore<u64>(rec + tid, 0ull);
            if (tid == 0) set_error(err + b, SHAFA_OUTSIDE_MODULE);
            continue;
        }
        const u32 nt = (u32)((n + TP_TILE - 1) / TP_TILE);
        const u64 *r = part + (u64)tbase[b] * ERR_WORDS;
        const u32 per = (nt + TP_THREADS - 1) / TP_THREADS;
        const u32 lo = (u32)tid * per < nt ? (u32)tid * per : nt, hi = lo + per < nt ? lo + per : nt;
        ErrAgg a = err_identity();
        for (u32 j = lo; j < hi; ++j) {
            u64 v[ERR_WORDS];
#pragma unroll
            for (u32 i = 0; i < ERR_WORDS; i += 2) {
                const uint4 x = gload<uint4>(r + (u64)j * ERR_WORDS + i);
                v[i] = (u64)x.y << 32 | x.x; v[i + 1] = (u64)x.w << 32 | x.z;
            }
            a = err_then(a, err_get(v));
        }
        a = err_wave_reduce(a);
        if (lane_id() == 0) err_put(&wres[wave_id()][0], a);
        lds_barrier();
        if (tid == 0) {
            ErrAgg t = err_waves(&wres[0][0]);
            if (t.xmin == 0.0) t.xmin = 0.0;         // a zero extreme is +0.0
            if (t.xmax == 0.0) t.xmax = 0.0;
            u64 v[ERR_WORDS];
            v[0] = n;
            err_put(v, t);
#pragma unroll
            for (u32 i = 0; i < ERR_WORDS; ++i) gstore<u64>(rec + i, v[i]);
        }
        lds_barrier();                               // the next block of this workgroup writes the wave results
    }
}

// ---- merge
// The three launches are templated on their SOURCE: LAG_PLANES the _lag entries' (d[i] unfolded from the planes),
// LAG_PLANES_SKIP the same where a block whose lag is 0 is another family's and skipped (the grid merge's first pass), LAG_ELEMS
// the elements themselves, in place: x[i] += x[i - L] with no planes and no unfold (the grid merge's further passes; a lag of 0:
// the block has no such pass).  A lane reads only the elements it writes, and the sums are taken in a launch of their own in
// front, so in place is safe.
enum LagSrc { LAG_PLANES = 0, LAG_PLANES_SKIP = 1, LAG_ELEMS = 2 };

// d[i], unfolded from byte i of the E planes at pl[0 .. E - 1]
template <int E>
__device__ __forceinline__ typename ElT<E>::T lag_d(const u8 *const (&pl)[E], u64 i)
{
    using T = typename ElT<E>::T;
    T z = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) z = (T)(z | (T)((T)gload<u8>(pl[j] + i) << (8 * j)));
    return (T)((T)(z >> 1) ^ (T)(0 - (z & 1)));
}

// d[i] of the source: unfolded from the planes, or element i of the region at el itself
template <int E, int SRC>
__device__ __forceinline__ typename ElT<E>::T lag_src(const u8 *const (&pl)[E], const u8 *el, u64 i)
{
    if (SRC == LAG_ELEMS) return gload<typename ElT<E>::T>(el + i * E);
    return lag_d<E>(pl, i);
}

// The walk all three launches share: every tile of the capacities is entered (the skips are by item, not by tile), and tile k of
// a block's nt takes the run [k count / nt, (k + 1) count / nt) of the block's `count` items or column runs.
struct LagRun {
    u64 lo, hi;
    __device__ __forceinline__ LagRun(const TpWalk &wk, u64 count)
    {
        // floor(k count / nt) without the product k count, which passes 64 bits for a lag and a capacity of 2^43 elements
        // or more: per k <= count, and rest k < nt^2 < 2^62
        const u64 nt = wk.tnext - wk.tb, per = count / nt, rest = count % nt;
        lo = per * wk.k + rest * wk.k / nt;
        hi = per * (wk.k + 1ull) + rest * (wk.k + 1ull) / nt;
    }
};

// launch 1: sums[chunk L + column] for every chunk with a chunk behind it in the block's d_n[b] elements (all its rows are whole)
template <int E, int SRC = LAG_PLANES>
__global__ __launch_bounds__(TP_THREADS) void planes_lag_sums(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                              const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                              const u64 *__restrict__ d_n, const u8 *__restrict__ d_planes,
                                                              const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                              u32 n_tiles, u32 per_wg, u8 *__restrict__ sums_all)
{
    using T = typename ElT<E>::T;
    __shared__ T seg[TP_THREADS];
    const u32 tid = threadIdx.x;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        wk.enter();
        if (!wk.n) continue;                         // (uniform) empty, or past its capacity
        if (SRC != LAG_PLANES && !d_lag[wk.b]) continue;                       // (uniform) not this pass's block
        const LagGeom g(cap[wk.b], d_lag[wk.b]);
        if (g.NC < 2) continue;                      // (uniform)
        const u64 rows = (wk.n + g.L - 1) / g.L;
        const LagRun run(wk, g.NI);
        T *sums = (T *)sums_all + (u64)wk.tb * LAG_SUMS_TILE;
        const u8 *pl[E];
#pragma unroll
        for (int j = 0; j < E; ++j) pl[j] = SRC == LAG_ELEMS ? nullptr : d_planes + d_poff[(u64)wk.b * E + j];
        const u32 s = tid / g.W, c = tid - s * g.W;
        for (u64 w = run.lo; w < run.hi; ++w) {
            const u64 ch = w / g.NS, col = (w - ch * g.NS) * g.W + c, row0 = ch * g.G;
            if (row0 + g.G >= rows) break;           // (uniform) the chunk the block ends in, or one behind it
            const bool act = s < g.S && col < g.L;
            T t = 0;
            if (act) {
                for (u32 q = 0; q < g.m; ++q) {
                    u64 i = (row0 + (u64)q * LAG_ROWS * g.S + (u64)s * LAG_ROWS) * g.L + col;
#pragma unroll 8
                    for (u32 k = 0; k < LAG_ROWS; ++k, i += g.L) t = (T)(t + lag_src<E, SRC>(pl, wk.in, i));
                }
            }
            if (g.S > 1) {                           // (uniform)
                seg[tid] = t;
                lds_barrier();
                if (s == 0 && act) {
                    t = 0;
                    for (u32 s2 = 0; s2 < g.S; ++s2) t = (T)(t + seg[s2 * g.W + c]);
                }
            }
            if (s == 0 && act) gstore<T>(sums + ch * g.L + col, t);
            if (g.S > 1) lds_barrier();              // the next item writes the segments' totals
        }
    }
}

// launch 2: down each column, the sums of the chunks in front of every chunk that holds a row of the block
template <int E, int SRC = LAG_PLANES>
__global__ __launch_bounds__(TP_THREADS) void planes_lag_scan(const u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                              const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                              const u64 *__restrict__ d_n, const u64 *__restrict__ d_lag,
                                                              u32 n_tiles, u32 per_wg, u8 *__restrict__ sums_all)
{
    using T = typename ElT<E>::T;
    __shared__ T seg[TP_THREADS];
    const u32 tid = threadIdx.x;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        wk.enter();
        if (!wk.n) continue;                         // (uniform)
        if (SRC != LAG_PLANES && !d_lag[wk.b]) continue;                       // (uniform) not this pass's block
        const LagGeom g(cap[wk.b], d_lag[wk.b]);
        if (g.NC < 2) continue;                      // (uniform)
        const u64 rows = (wk.n + g.L - 1) / g.L, nc = (rows + g.G - 1) / g.G;      // the chunks that hold a row
        if (nc < 2) continue;                        // (uniform) the merge reads no prefix
        const u32 w2 = g.L < LAG_SCAN_COLS ? (u32)g.L : LAG_SCAN_COLS, gs_n = TP_THREADS / w2;
        const LagRun run(wk, (g.L + w2 - 1) / w2);
        T *sums = (T *)sums_all + (u64)wk.tb * LAG_SUMS_TILE;
        const u32 gs = tid / w2, c = tid - gs * w2;
        for (u64 cr = run.lo; cr < run.hi; ++cr) {
            const u64 col = cr * w2 + c;
            const bool act = gs < gs_n && col < g.L;
            T carry = 0;
            for (u64 at = 0; at < nc; at += (u64)gs_n * LAG_SCAN_PER) {         // (uniform)
                const u64 ch0 = at + (u64)gs * LAG_SCAN_PER;
                T v[LAG_SCAN_PER], t = 0;
#pragma unroll
                for (u32 q = 0; q < LAG_SCAN_PER; ++q) v[q] = act && ch0 + q + 1 < nc ? gload<T>(sums + (ch0 + q) * g.L + col) : (T)0;
#pragma unroll
                for (u32 q = 0; q < LAG_SCAN_PER; ++q) {
                    const T x = v[q];
                    v[q] = t;
                    t = (T)(t + x);
                }
                seg[tid] = t;
                lds_barrier();
                T pre = carry, tot = 0;
                for (u32 g2 = 0; g2 < gs_n; ++g2) {
                    const T x = seg[g2 * w2 + c];
                    if (g2 < gs) pre = (T)(pre + x);
                    tot = (T)(tot + x);
                }
                lds_barrier();                       // the next round writes the lanes' totals
                carry = (T)(carry + tot);
#pragma unroll
                for (u32 q = 0; q < LAG_SCAN_PER; ++q)
                    if (act && ch0 + q < nc) gstore<T>(sums + (ch0 + q) * g.L + col, (T)(pre + v[q]));
            }
        }
    }
}

// ---- the strips of 256 columns (L >= LAG_STRIP) in launch 3: a lane takes FOUR columns next to each other and LAG_ROWS / 4 rows
// of the round's LAG_ROWS, so a plane is read a dword a lane (a wave: 256 contiguous bytes of one row, at any alignment) and the
// elements leave four at a time; the four groups of rows are chained through LDS as the segments of the narrow form are.
constexpr u32 LAG_VEC = 4, LAG_VROWS = LAG_ROWS / LAG_VEC;
typedef u32 u32_any_t __attribute__((aligned(1)));
typedef u32x2_t u32x2_any_t __attribute__((aligned(2)));
typedef u32x4_t u32x4_any_t __attribute__((aligned(4)));

// four elements next to each other to p, a multiple of E: one store (two at 8 bytes) at the element's alignment
template <int E>
__device__ __forceinline__ void lag_store4(u8 *p, const typename ElT<E>::T (&v)[LAG_VEC])
{
    const unsigned long long a = (unsigned long long)p;
    if (E == 1) *(GLOBAL_AS u32_any_t *)a = (u32)v[0] | (u32)v[1] << 8 | (u32)v[2] << 16 | (u32)v[3] << 24;
    else if (E == 2) {
        u32x2_t x;
        x.x = (u32)v[0] | (u32)v[1] << 16; x.y = (u32)v[2] | (u32)v[3] << 16;
        *(GLOBAL_AS u32x2_any_t *)a = x;
    } else if (E == 4) {
        u32x4_t x;
        x.x = (u32)v[0]; x.y = (u32)v[1]; x.z = (u32)v[2]; x.w = (u32)v[3];
        *(GLOBAL_AS u32x4_any_t *)a = x;
    } else {
        u32x4_t x, y;
        x.x = (u32)v[0]; x.y = (u32)((u64)v[0] >> 32); x.z = (u32)v[1]; x.w = (u32)((u64)v[1] >> 32);
        y.x = (u32)v[2]; y.y = (u32)((u64)v[2] >> 32); y.z = (u32)v[3]; y.w = (u32)((u64)v[3] >> 32);
        *(GLOBAL_AS u32x4_any_t *)a = x;
        *(GLOBAL_AS u32x4_any_t *)(a + 16) = y;
    }
}

// d[i .. i + 3] (all four inside the block and the row) from one dword of each plane
template <int E>
__device__ __forceinline__ void lag_d4(const u8 *const (&pl)[E], u64 i, typename ElT<E>::T (&d)[LAG_VEC])
{
    using T = typename ElT<E>::T;
    u32 w[E];
#pragma unroll
    for (int j = 0; j < E; ++j) w[j] = *(const GLOBAL_AS u32_any_t *)(unsigned long long)(pl[j] + i);
#pragma unroll
    for (u32 c = 0; c < LAG_VEC; ++c) {
        T z = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) z = (T)(z | (T)((T)((w[j] >> (8 * c)) & 0xFFu) << (8 * j)));
        d[c] = (T)((T)(z >> 1) ^ (T)(0 - (z & 1)));
    }
}

// d[i .. i + 3] of the source: lag_d4, or the four elements at el + i E themselves (a multiple of E, as lag_store4's)
template <int E, int SRC>
__device__ __forceinline__ void lag_src4(const u8 *const (&pl)[E], const u8 *el, u64 i, typename ElT<E>::T (&d)[LAG_VEC])
{
    using T = typename ElT<E>::T;
    if (SRC != LAG_ELEMS) {
        lag_d4<E>(pl, i, d);
        return;
    }
    const unsigned long long a = (unsigned long long)(el + i * E);
    if (E == 1) {
        const u32 x = *(const GLOBAL_AS u32_any_t *)a;
#pragma unroll
        for (u32 c = 0; c < LAG_VEC; ++c) d[c] = (T)(x >> (8 * c));
    } else if (E == 2) {
        const u32x2_t x = *(const GLOBAL_AS u32x2_any_t *)a;
        d[0] = (T)x.x; d[1] = (T)(x.x >> 16); d[2] = (T)x.y; d[3] = (T)(x.y >> 16);
    } else if (E == 4) {
        const u32x4_t x = *(const GLOBAL_AS u32x4_any_t *)a;
        d[0] = (T)x.x; d[1] = (T)x.y; d[2] = (T)x.z; d[3] = (T)x.w;
    } else {
        const u32x4_t x = *(const GLOBAL_AS u32x4_any_t *)a, y = *(const GLOBAL_AS u32x4_any_t *)(a + 16);
        d[0] = (T)((u64)x.y << 32 | x.x); d[1] = (T)((u64)x.w << 32 | x.z);
        d[2] = (T)((u64)y.y << 32 | y.x); d[3] = (T)((u64)y.w << 32 | y.z);
    }
}

// one chunk of a strip of 256 columns from row row0 on: every lane of the workgroup calls (the barriers); m, rows, n uniform
template <int E, int SRC>
__device__ __forceinline__ void lag_merge_wide(const u8 *const (&pl)[E], u8 *dst, u64 n, u64 L, u64 rows, u64 row0, u32 m, u64 strip0,
                                               const typename ElT<E>::T *prefix, typename ElT<E>::T *seg)
{
    using T = typename ElT<E>::T;
    const u32 tid = threadIdx.x, rg = tid >> 6, cl = tid & 63u;
    const u64 col0 = strip0 + (u64)cl * LAG_VEC;
    const bool whole = col0 + LAG_VEC <= L;          // the lane's four columns are all the row's
    T acc[LAG_VEC];
#pragma unroll
    for (u32 c = 0; c < LAG_VEC; ++c) acc[c] = prefix && col0 + c < L ? gload<T>(prefix + col0 + c) : (T)0;
    for (u32 q = 0; q < m; ++q) {
        const u64 rq = row0 + (u64)q * LAG_ROWS;
        if (rq >= rows) break;                       // (uniform)
        const u64 i0 = (rq + (u64)rg * LAG_VROWS) * L + col0;
        T d[LAG_VROWS][LAG_VEC];
        {
            u64 i = i0;
#pragma unroll
            for (u32 k = 0; k < LAG_VROWS; ++k, i += L) {
                if (whole && i + LAG_VEC <= n) lag_src4<E, SRC>(pl, dst, i, d[k]);
                else {
#pragma unroll
                    for (u32 c = 0; c < LAG_VEC; ++c) d[k][c] = col0 + c < L && i + c < n ? lag_src<E, SRC>(pl, dst, i + c) : (T)0;
                }
            }
        }
#pragma unroll
        for (u32 k = 1; k < LAG_VROWS; ++k)
#pragma unroll
            for (u32 c = 0; c < LAG_VEC; ++c) d[k][c] = (T)(d[k][c] + d[k - 1][c]);
#pragma unroll
        for (u32 c = 0; c < LAG_VEC; ++c) seg[tid * LAG_VEC + c] = d[LAG_VROWS - 1][c];
        lds_barrier();
        T pre[LAG_VEC];
#pragma unroll
        for (u32 c = 0; c < LAG_VEC; ++c) {
            pre[c] = acc[c];
#pragma unroll
            for (u32 g2 = 0; g2 < LAG_VEC; ++g2) {
                const T x = seg[(g2 * 64u + cl) * LAG_VEC + c];
                if (g2 < rg) pre[c] = (T)(pre[c] + x);
                acc[c] = (T)(acc[c] + x);
            }
        }
        lds_barrier();                               // the next round writes the groups' totals
        {
            u64 i = i0;
#pragma unroll
            for (u32 k = 0; k < LAG_VROWS; ++k, i += L) {
                if (whole && i + LAG_VEC <= n) {
                    T o[LAG_VEC];
#pragma unroll
                    for (u32 c = 0; c < LAG_VEC; ++c) o[c] = (T)(pre[c] + d[k][c]);
                    lag_store4<E>(dst + i * E, o);
                } else {
#pragma unroll
                    for (u32 c = 0; c < LAG_VEC; ++c)
                        if (col0 + c < L && i + c < n) gstore<T>(dst + (i + c) * E, (T)(pre[c] + d[k][c]));
                }
            }
        }
    }
}

// launch 3: sums[chunk L + column] is by now the sum of the column's d's in front of the chunk (have_sums: launches 1 and 2 ran)
template <int E, int SRC = LAG_PLANES>
__global__ __launch_bounds__(TP_THREADS) void planes_lag_merge(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                               const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                               const u64 *__restrict__ d_n, const u8 *__restrict__ d_planes,
                                                               const u64 *__restrict__ d_poff, const u64 *__restrict__ d_lag,
                                                               int *__restrict__ err, u32 n_tiles, u32 per_wg,
                                                               const u8 *__restrict__ sums_all)
{
    using T = typename ElT<E>::T;
    __shared__ T seg[TP_THREADS * LAG_VEC];
    const u32 tid = threadIdx.x;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        wk.enter();
        const u64 n = wk.n;
        if (!n) continue;                            // (uniform) empty, or past its capacity: no byte of it is touched
        if (SRC != LAG_PLANES && !d_lag[wk.b]) continue;                       // (uniform) not this pass's block
        const LagGeom g(cap[wk.b], d_lag[wk.b]);
        const u64 rows = (n + g.L - 1) / g.L;
        const bool chained = (rows + g.G - 1) / g.G > 1;                         // (uniform) planes_lag_scan's condition
        const LagRun run(wk, g.NI);
        const T *sums = (const T *)sums_all + (u64)wk.tb * LAG_SUMS_TILE;
        u8 *dst = (u8 *)wk.in;
        const u8 *pl[E];
#pragma unroll
        for (int j = 0; j < E; ++j) pl[j] = SRC == LAG_ELEMS ? nullptr : d_planes + d_poff[(u64)wk.b * E + j];
        const u32 s = tid / g.W, c = tid - s * g.W;
        for (u64 w = run.lo; w < run.hi; ++w) {
            const u64 ch = w / g.NS, col = (w - ch * g.NS) * g.W + c, row0 = ch * g.G;
            if (row0 >= rows) break;                 // (uniform) behind the block's last row
            if (g.W == LAG_STRIP) {                  // (uniform) four columns a lane
                lag_merge_wide<E, SRC>(pl, dst, n, g.L, rows, row0, g.m, (w - ch * g.NS) * g.W, chained ? sums + ch * g.L : nullptr, seg);
                continue;
            }
            const bool act = s < g.S && col < g.L;
            T acc = chained && act ? gload<T>(sums + ch * g.L + col) : (T)0;     // the element above the round's first row
            for (u32 q = 0; q < g.m; ++q) {
                const u64 rq = row0 + (u64)q * LAG_ROWS * g.S;
                if (rq >= rows) break;               // (uniform)
                const u64 i0 = (rq + (u64)s * LAG_ROWS) * g.L + col;
                T d[LAG_ROWS];
                {
                    u64 i = i0;
#pragma unroll
                    for (u32 k = 0; k < LAG_ROWS; ++k, i += g.L) d[k] = act && i < n ? lag_src<E, SRC>(pl, dst, i) : (T)0;
                }
#pragma unroll
                for (u32 k = 1; k < LAG_ROWS; ++k) d[k] = (T)(d[k] + d[k - 1]);
                T pre = acc;
                if (g.S > 1) {                       // (uniform) the segments above this one in the round
                    seg[tid] = d[LAG_ROWS - 1];
                    lds_barrier();
                    T tot = 0;
                    for (u32 s2 = 0; s2 < g.S; ++s2) {
                        const T x = seg[s2 * g.W + c];
                        if (s2 < s) pre = (T)(pre + x);
                        tot = (T)(tot + x);
                    }
                    lds_barrier();                   // the next round writes the segments' totals
                    acc = (T)(acc + tot);
                } else acc = (T)(acc + d[LAG_ROWS - 1]);
                {
                    u64 i = i0;
#pragma unroll
                    for (u32 k = 0; k < LAG_ROWS; ++k, i += g.L)
                        if (act && i < n) gstore<T>(dst + i * E, (T)(pre + d[k]));
                }
            }
        }
    }
    tp_size_errors(cap, d_n, nblk, err);
}

// ---- behind the grid merge of an error-bounded field: the codes, in place, -> T(code) (x) step, then the outliers'
// own bits on top.
// the restore of the tile wk has entered, for the quantised and the rounded field: a tile's elements lie in whole 16-byte words
// of the address space but for the word the tile starts in and the one it ends in (the element side is at multiples of E, so an
// element never straddles two words): a lane takes every 256th word, one 16-byte load and store with word(x) on its four u32 in
// between, and the elements of a cut word one by one, elem(p) on the element at p.
template <int E, class Word, class Elem>
__device__ __forceinline__ void restore_tile(const TpWalk &wk, Word word, Elem elem)
{
    const u64 end = wk.pos0 + TP_TILE < wk.n ? wk.pos0 + TP_TILE : wk.n;
    const u64 lo = (u64)(uintptr_t)wk.in + wk.pos0 * E, hi = (u64)(uintptr_t)wk.in + end * E;          // the tile's bytes
    for (u64 a = (lo & ~(u64)15) + 16ull * threadIdx.x; a < hi; a += 16ull * TP_THREADS) {
        u8 *p = (u8 *)(uintptr_t)a;
        if (a >= lo && a + 16 <= hi) {
            const uint4 v = gload<uint4>(p);
            u32 x[4] = {v.x, v.y, v.z, v.w};
            word(x);
            gstore<uint4>(p, make_uint4(x[0], x[1], x[2], x[3]));
        } else {
#pragma unroll
            for (u32 i = 0; i < 16 / E; ++i) {
                const u64 at = a + (u64)i * E;
                if (at >= lo && at < hi) elem(p + i * E);
            }
        }
    }
}

// d_step: the bits of the blocks' steps as T
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_field_restore(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                   const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                                   const u64 *__restrict__ d_n, const u64 *__restrict__ d_step,
                                                                   u32 n_tiles, u32 per_wg)
{
    using U = typename FieldT<E>::U;
    using I = typename FieldT<E>::I;
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const typename FieldT<E>::F step = field_bits<E>(d_step[wk.b]);
        restore_tile<E>(
            wk,
            [&](u32 (&x)[4]) {
#pragma unroll
                for (u32 i = 0; i < 16 / E; ++i) {
                    const I code = E == 8 ? (I)((u64)x[(2 * i + 1) & 3] << 32 | x[(2 * i) & 3]) : (I)x[i];
                    const u64 y = (u64)__builtin_bit_cast(U, field_value<E>(code, step));
                    if (E == 8) { x[(2 * i) & 3] = (u32)y; x[(2 * i + 1) & 3] = (u32)(y >> 32); }
                    else x[i] = (u32)y;
                }
            },
            [&](u8 *p) { gstore<U>(p, __builtin_bit_cast(U, field_value<E>((I)gload<U>(p), step))); });
    }
}

// ---- behind the grid merge of a rounded field: restore_tile with round_value for the restorer, eight elements a
// 16-byte word at E = 2.  d_q: the blocks' d | mant << 8.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_round_restore(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                   const u64 *__restrict__ cap, const u32 *__restrict__ tbase, int nblk,
                                                                   const u64 *__restrict__ d_n, const u64 *__restrict__ d_q,
                                                                   u32 n_tiles, u32 per_wg)
{
    using U = typename RoundT<E>::U;
    using S = typename ElT<E>::T;                    // an element as it is stored
    for (TpWalk wk(d_el, off, cap, tbase, nblk, d_n, n_tiles, per_wg); wk.more(); wk.step()) {
        if (!wk.enter()) continue;
        const u32 d = (u32)d_q[wk.b] & 0xFFu;
        restore_tile<E>(
            wk,
            [&](u32 (&x)[4]) {
#pragma unroll
                for (u32 i = 0; i < 4; ++i) {
                    if (E == 8) {
                        if (i & 1) {
                            const u64 y = (u64)round_value<E>((U)((u64)x[i] << 32 | x[i - 1]), d);
                            x[i - 1] = (u32)y; x[i] = (u32)(y >> 32);
                        }
                    } else if (E == 4) x[i] = (u32)round_value<E>((U)x[i], d);
                    else x[i] = (u32)round_value<E>((U)(x[i] & 0xFFFFu), d) | (u32)round_value<E>((U)(x[i] >> 16), d) << 16;
                }
            },
            [&](u8 *p) { gstore<S>(p, (S)round_value<E>((U)gload<S>(p), d)); });
    }
}

// the patch: one thread a record.  first[b]: the number of block b's first record among the call's (first[nblk]: their count);
// rec_off[b]: its first record in d_outl.  A position at or past the block's size (a block past its capacity has none) is the
// block's SHAFA_OUTSIDE_MODULE and nothing is written for it.
template <int E>
__global__ __launch_bounds__(TP_THREADS) void planes_field_patch(u8 *__restrict__ d_el, const u64 *__restrict__ off,
                                                                 const u64 *__restrict__ cap, int nblk, const u64 *__restrict__ d_n,
                                                                 const u64 *__restrict__ rec_off, const u64 *__restrict__ first,
                                                                 const u64 *__restrict__ d_outl, int *__restrict__ err)
{
    const u64 total = first[nblk];
    for (u64 i = (u64)blockIdx.x * TP_THREADS + threadIdx.x; i < total; i += (u64)gridDim.x * TP_THREADS) {
        int lo = 0, hi = nblk;                       // first[lo] <= i, the record's block in [lo, hi)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (first[mid] <= i) lo = mid;
            else hi = mid;
        }
        const u64 *rec = d_outl + 2 * (rec_off[lo] + (i - first[lo]));
        const u64 pos = gload<u64>(rec), n = d_n[lo] > cap[lo] ? 0 : d_n[lo];
        if (pos >= n) {
            set_error(err + lo, SHAFA_OUTSIDE_MODULE);
            continue;
        }
        gstore<typename FieldT<E>::U>(d_el + off[lo] + pos * E, (typename FieldT<E>::U)gload<u64>(rec + 1));
    }
}

// the launches read tile_setup's workspace: extra 0 the plane offsets, extra 1 the clamped lags, the scratch the column sums
template <int E>
void planes_lag_launch(bool merge, bool sums, const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n, u8 *d_planes,
                       int *err)
{
    const u64 *poff = (const u64 *)a.extra[0], *lag = (const u64 *)a.extra[1];
    if (!merge) {
        hipLaunchKernelGGL(planes_lag_split<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblk,
                           d_n, d_planes, poff, lag, err, a.nt, a.per_wg);
        return;
    }
    if (sums) {
        hipLaunchKernelGGL(planes_lag_sums<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblk,
                           d_n, (const u8 *)d_planes, poff, lag, a.nt, a.per_wg, a.scratch);
        hipLaunchKernelGGL(planes_lag_scan<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblk,
                           d_n, lag, a.nt, a.per_wg, a.scratch);
    }
    hipLaunchKernelGGL(planes_lag_merge<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblk, d_n,
                       (const u8 *)d_planes, poff, lag, err, a.nt, a.per_wg, (const u8 *)a.scratch);
}

// one pass of the lag family over the blocks whose lag in the row `lag` is not 0: the sums and their scan where a block of the
// pass has more than one chunk, then the merge
template <int E, int SRC>
void planes_lag_pass(bool sums, const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n, const u8 *d_planes,
                     const u64 *poff, const u64 *lag, int *err)
{
    if (sums) {
        hipLaunchKernelGGL((planes_lag_sums<E, SRC>), dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase,
                           nblk, d_n, d_planes, poff, lag, a.nt, a.per_wg, a.scratch);
        hipLaunchKernelGGL((planes_lag_scan<E, SRC>), dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase,
                           nblk, d_n, lag, a.nt, a.per_wg, a.scratch);
    }
    hipLaunchKernelGGL((planes_lag_merge<E, SRC>), dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblk, d_n,
                       d_planes, poff, lag, err, a.nt, a.per_wg, (const u8 *)a.scratch);
}

// what the host knows of a grid merge's passes: which are made at all, and which of them have a block of more than one chunk
struct GridPlan {
    bool diff, first, first_sums, pass[SHAFA_PLANES_GRID_LAGS], pass_sums[SHAFA_PLANES_GRID_LAGS];
};

// the launches read tile_setup's workspace: extra 0 the plane offsets, extra 1 the rows of lags (planes_grid_launch_dev), the
// scratch the sums of whichever pass is running
template <int E>
void planes_grid_launch(bool merge, const GridPlan &gp, const TileSetup &a, hipStream_t st, u8 *d_el, int nblk, const u64 *d_n,
                        u8 *d_planes, int *err)
{
    const u64 *poff = (const u64 *)a.extra[0], *lag = (const u64 *)a.extra[1];
    if (!merge) {
        hipLaunchKernelGGL(planes_grid_split<E>, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblk,
                           d_n, d_planes, poff, lag, err, a.nt, a.per_wg);
        return;
    }
    if (gp.diff) planes_diff_merge_enqueue(E, a, st, d_el, nblk, d_n, d_planes, err, lag);
    if (gp.first) planes_lag_pass<E, LAG_PLANES_SKIP>(gp.first_sums, a, st, d_el, nblk, d_n, d_planes, poff, lag, err);
    for (int k = 1; k < SHAFA_PLANES_GRID_LAGS; ++k)
        if (gp.pass[k])
            planes_lag_pass<E, LAG_ELEMS>(gp.pass_sums[k], a, st, d_el, nblk, d_n, nullptr, poff, lag + (size_t)k * nblk, err);
}

// a double that is exactly a T -> T's bits; T(1 / step), the double division rounded to T once
u64 field_bits_of(u32 elem, double v)
{
    if (elem == 8) return __builtin_bit_cast(u64, v);
    return __builtin_bit_cast(u32, (float)v);
}

// the blocks' lags, nlags slots a block -> SHAFA_PLANES_GRID_LAGS rows of nb lags at `rows` (zeroed by the caller): a slot at or past
// the block's capacity subtracts nothing and goes as 0, as an unused one does
void grid_lag_rows(u64 *rows, size_t nb, const u64 *h_cap, u32 nlags, const u64 *h_lags)
{
    for (size_t b = 0; b < nb; ++b)
        for (u32 k = 0; k < nlags; ++k) {
            const u64 g = h_lags[b * nlags + k];
            rows[k * nb + b] = g < h_cap[b] ? g : 0;
        }
}

// a quantiser's device rows of nb words at q, as FieldQ, RoundQ and ErrQ read them.  h_mant non-NULL: the rounding's one row,
// d | mant << 8.  Else the bits of the steps as T and, where the caller has bounds (the merge has none), two more rows: the bits
// of 1 / step and of the bounds
void quant_rows(u64 *q, size_t nb, u32 elem, const double *h_step, const double *h_bound, const u32 *h_mant, const u32 *h_keep)
{
    for (size_t b = 0; b < nb; ++b) {
        if (h_mant) {
            q[b] = (u64)(h_mant[b] - h_keep[b]) | (u64)h_mant[b] << 8;
            continue;
        }
        q[b] = field_bits_of(elem, h_step[b]);
        if (!h_bound) continue;
        q[nb + b] = field_bits_of(elem, field_inverse(elem, h_step[b]));
        q[2 * nb + b] = field_bits_of(elem, h_bound[b]);
    }
}

}  // namespace

double field_inverse(u32 elem, double step) { return elem == 8 ? 1.0 / step : (double)(float)(1.0 / step); }

// the _grid entries.  h_lags: nlags slots a block, checked by the caller (the first >= 1, the others 0 or
// increasing).  The device gets SHAFA_PLANES_GRID_LAGS rows of nblocks lags, a slot at or past the block's capacity (it subtracts
// nothing) and an unused one as 0.  split: one launch.  merge: row 0 is the lag family's first pass, planes -> elements at the
// block's smallest lag, clamped as the _lag entries clamp it, and 0 where that lag is 1: those blocks are the _diff merge's, which
// skips the others; rows 1 and 2 are the passes in place over the elements.  All passes share one scratch, the stream their order.
// fq->round (the _grid_round entries): the same rows with d | mant << 8 for the step's bits, the inverse's and the
// bound's rows unused, and the rounding kernels for the quantising ones.
// fq (the _grid_quant entries): the same upload carries, behind the rows of lags, the quantiser's rows (quant_rows) — split: the
// bits of step, 1 / step and bound as T, the first record and the capacity of every block; merge: the steps' bits, the first
// records and the nblocks + 1 running counts of the records.
int planes_grid_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                           const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, u32 nlags, const u64 *h_lags,
                           const FieldQuant *fq)
{
    const size_t nb = (size_t)nblocks;
    std::vector<u64> lag(nb * SHAFA_PLANES_GRID_LAGS + (fq ? nb * 5 + 1 : 0), 0);
    GridPlan gp = {};
    u64 records = 0;
    if (fq) {                                        // the rows behind the lags: planes_grid_quant_split's, or the merge's
        u64 *q = lag.data() + nb * SHAFA_PLANES_GRID_LAGS;
        quant_rows(q, nb, elem, fq->h_step, merge ? nullptr : fq->h_bound, fq->round ? fq->h_mant : nullptr, fq->h_keep);
        for (size_t b = 0; b < nb; ++b) {
            if (!merge) {
                q[3 * nb + b] = fq->h_outl_off[b];
                q[4 * nb + b] = fq->h_outl_count[b];
            } else {                                 // the records' places, then the nb + 1 running counts of them
                q[nb + b] = fq->h_outl_off[b];
                q[2 * nb + b] = records;
                records += fq->h_outl_count[b];
            }
        }
        if (merge) q[3 * nb] = records;
    }
    grid_lag_rows(lag.data(), nb, h_cap, nlags, h_lags);
    for (size_t b = 0; merge && b < nb; ++b) {
        const u64 cap = h_cap[b];
        const u64 first = lag[b] ? lag[b] : cap ? cap : 1;
        if (first == 1) {
            gp.diff = true;
            lag[b] = 0;
        } else {
            gp.first = true;
            lag[b] = first;
            if (cap && LagGeom(cap, first).NC > 1) gp.first_sums = true;
        }
        for (int k = 1; k < SHAFA_PLANES_GRID_LAGS; ++k)
            if (lag[k * nb + b]) {
                gp.pass[k] = true;
                if (LagGeom(cap, lag[k * nb + b]).NC > 1) gp.pass_sums[k] = true;
            }
    }
    const bool sums = gp.first_sums || gp.pass_sums[1] || gp.pass_sums[2];
    static_assert(SHAFA_PLANES_GRID_LAGS == 3, "the passes named here");
    const TileExtra x[2] = {{h_plane_off, nb * elem * 8}, {lag.data(), lag.size() * 8}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, x, 2, sums ? (size_t)LAG_SUMS_TILE * elem : gp.diff ? 8 : 0, 0, &a))
        return rc;
    if (!a.wgs) a.wgs = 1;                           // without a tile one workgroup still looks for blocks past a capacity of 0
    // the quantising kernels exist at 4 and 8 bytes, the rounding ones at 2 as well; both read their rows behind the rows of lags
    if (fq && !merge) {
        using Split = void (*)(const u8 *, const u64 *, const u64 *, const u32 *, int, const u64 *, u8 *, const u64 *, const u64 *,
                               int *, u32, u32, u64 *, u64 *);
        Split split;
        if (fq->round && elem == 2) split = planes_grid_round_split<2>;
        else if (fq->round) split = elem == 4 ? planes_grid_round_split<4> : planes_grid_round_split<8>;
        else split = elem == 4 ? planes_grid_quant_split<4> : planes_grid_quant_split<8>;
        HIP_TRY(hipMemsetAsync(fq->d_outl_n, 0, nb * sizeof(u64), st));
        hipLaunchKernelGGL(split, dim3(a.wgs), dim3(TP_THREADS), 0, st, (const u8 *)d_el, a.off, a.cap, a.tbase, nblocks, d_n, d_planes,
                           (const u64 *)a.extra[0], (const u64 *)a.extra[1], bt->d_err, a.nt, a.per_wg, fq->d_outl, fq->d_outl_n);
        HIP_TRY(hipGetLastError());
        return SHAFA_SUCCESS;
    }
    switch (elem) {
    case 1: planes_grid_launch<1>(merge, gp, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 2: planes_grid_launch<2>(merge, gp, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 4: planes_grid_launch<4>(merge, gp, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    default: planes_grid_launch<8>(merge, gp, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    }
    if (fq) {                                        // the codes -> the values or the rounded bits in place, then the outliers on top
        using Restore = void (*)(u8 *, const u64 *, const u64 *, const u32 *, int, const u64 *, const u64 *, u32, u32);
        using Patch = void (*)(u8 *, const u64 *, const u64 *, int, const u64 *, const u64 *, const u64 *, const u64 *, int *);
        Restore restore;
        Patch patch;
        switch (elem) {
        case 2: restore = planes_round_restore<2>, patch = planes_field_patch<2>; break;
        case 4: restore = planes_round_restore<4>, patch = planes_field_patch<4>; break;
        default: restore = planes_round_restore<8>, patch = planes_field_patch<8>; break;
        }
        if (!fq->round) restore = elem == 4 ? planes_field_restore<4> : planes_field_restore<8>;
        const u64 *q = (const u64 *)a.extra[1] + nb * SHAFA_PLANES_GRID_LAGS;    // steps or d | mant << 8, record places, running counts
        hipLaunchKernelGGL(restore, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblocks, d_n, q, a.nt, a.per_wg);
        const u64 wgs = (records + TP_THREADS - 1) / TP_THREADS;
        if (records)
            hipLaunchKernelGGL(patch, dim3((u32)(wgs < TP_MAX_WGS ? wgs : TP_MAX_WGS)), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap,
                               nblocks, d_n, q + nb, q + 2 * nb, fq->d_outl, bt->d_err);
    }
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// the hist entries of the _grid family: shafa_hipd_hist_planes_grid_dev without fq, and with it
// shafa_hipd_hist_planes_grid_quant_dev or, fq->round, shafa_hipd_hist_planes_grid_round_dev; of fq
// the quantiser's parameters and d_outl_n are looked at.  h_lags as the _grid entries', checked by the caller; without fq a row
// of zeros is allowed: plain planes.  The device gets the grid split's rows of clamped lags and behind them, without fq, a fourth
// row, 1 where the block's row is not all zeros, else the quantiser's rows as the split gets them.  The grid is this launcher's
// own: a workgroup a run of SHAFA_PLANES_HIST_RUN consecutive tiles.  One memset, with fq a second one of d_outl_n, one launch.
int planes_grid_hist_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, const u8 *d_el, const u64 *h_off, const u64 *h_cap,
                                const u64 *d_n, u32 nlags, const u64 *h_lags, const FieldQuant *fq, u64 *d_freq)
{
    const size_t nb = (size_t)nblocks;
    std::vector<u64> lag(nb * (SHAFA_PLANES_GRID_LAGS + (fq && !fq->round ? 3 : 1)), 0);
    u64 *q = lag.data() + nb * SHAFA_PLANES_GRID_LAGS;
    grid_lag_rows(lag.data(), nb, h_cap, nlags, h_lags);
    if (fq) quant_rows(q, nb, elem, fq->h_step, fq->h_bound, fq->round ? fq->h_mant : nullptr, fq->h_keep);
    else
        for (size_t b = 0; b < nb; ++b) q[b] = h_lags[b * nlags] != 0;    // a row that is not all zeros starts with a lag
    const TileExtra x[1] = {{lag.data(), lag.size() * 8}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, x, 1, 0, 0, &a)) return rc;
    HIP_TRY(hipMemsetAsync(d_freq, 0, nb * elem * 256 * sizeof(u64), st));
    const u32 wgs = a.nt ? (a.nt + GH_RUN - 1) / GH_RUN : 1;    // without a tile one workgroup still looks for blocks past a capacity of 0
    if (!fq) {
        auto kernel = elem == 1 ? planes_grid_hist<1> : elem == 2 ? planes_grid_hist<2> : elem == 4 ? planes_grid_hist<4> : planes_grid_hist<8>;
        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblocks, d_n,
                           (const u64 *)a.extra[0], bt->d_err, a.nt, d_freq);
    } else {
        HIP_TRY(hipMemsetAsync(fq->d_outl_n, 0, nb * sizeof(u64), st));
        auto kernel = elem == 4 ? planes_grid_quant_hist<4> : planes_grid_quant_hist<8>;
        if (fq->round) kernel = elem == 2 ? planes_grid_round_hist<2> : elem == 4 ? planes_grid_round_hist<4> : planes_grid_round_hist<8>;
        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblocks, d_n,
                           (const u64 *)a.extra[0], bt->d_err, a.nt, d_freq, fq->d_outl_n);
    }
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// the _lag entries: split is one launch; merge is the column sums and their scan (where a block has more than one chunk) and the
// merge itself.  The caller has checked the arguments (every h_lag[b] >= 1).
int planes_lag_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                          const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, const u64 *h_lag)
{
    std::vector<u64> lag((size_t)nblocks);
    bool sums = false;
    for (int b = 0; b < nblocks; ++b) {
        lag[b] = h_lag[b] < h_cap[b] ? h_lag[b] : h_cap[b] ? h_cap[b] : 1;       // at or past the capacity: no element has a base
        if (merge && h_cap[b] && LagGeom(h_cap[b], lag[b]).NC > 1) sums = true;
    }
    const TileExtra x[2] = {{h_plane_off, (size_t)nblocks * elem * 8}, {lag.data(), (size_t)nblocks * 8}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, x, 2, sums ? (size_t)LAG_SUMS_TILE * elem : 0, 0, &a)) return rc;
    if (!a.wgs) a.wgs = 1;                           // without a tile one workgroup still looks for blocks past a capacity of 0
    switch (elem) {
    case 1: planes_lag_launch<1>(merge, sums, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 2: planes_lag_launch<2>(merge, sums, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    case 4: planes_lag_launch<4>(merge, sums, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    default: planes_lag_launch<8>(merge, sums, a, st, d_el, nblocks, d_n, d_planes, bt->d_err); break;
    }
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

// the error entries.  The arguments have been checked by the caller.  The device gets three rows of nblocks words,
// ErrQ's, and for shafa_hipd_error_dev the offsets of the originals; the scratch is one partial of SHAFA_ERR_WORDS words per tile
// of the capacities.  Two launches: the tiles (where there is one), then one workgroup a block.
int planes_error_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, const ErrorArgs &e, const u8 *d_el, const u64 *h_off,
                            const u64 *h_cap, const u64 *d_n, u64 *d_stat)
{
    const size_t nb = (size_t)nblocks;
    std::vector<u64> q(nb * 3, 0);
    if (e.src != ERR_PAIR) quant_rows(q.data(), nb, elem, e.h_step, e.h_bound, e.src == ERR_ROUND ? e.h_mant : nullptr, e.h_keep);
    else
        for (size_t b = 0; b < nb; ++b) {
            q[b] = e.h_mant[b];
            q[nb + b] = __builtin_bit_cast(u64, e.h_abs[b]);
            q[2 * nb + b] = __builtin_bit_cast(u64, e.h_rel[b]);
        }
    const TileExtra x[2] = {{q.data(), q.size() * 8}, {e.h_ref_off, nb * 8}};
    TileSetup a;
    if (int rc = tile_setup(bt, st, nblocks, h_off, h_cap, TP_TILE, x, 2, ERR_WORDS * sizeof(u64), 0, &a)) return rc;
    using Tiles = void (*)(const u8 *, const u64 *, const u64 *, const u32 *, int, const u64 *, const u8 *, const u64 *, const u64 *,
                           u64 *, u32, u32);
    Tiles tiles;
    if (e.src == ERR_PAIR)
        tiles = elem == 2 ? planes_error_tiles<2, ERR_PAIR> : elem == 4 ? planes_error_tiles<4, ERR_PAIR> : planes_error_tiles<8, ERR_PAIR>;
    else if (e.src == ERR_QUANT) tiles = elem == 4 ? planes_error_tiles<4, ERR_QUANT> : planes_error_tiles<8, ERR_QUANT>;
    else tiles = elem == 2 ? planes_error_tiles<2, ERR_ROUND> : elem == 4 ? planes_error_tiles<4, ERR_ROUND> : planes_error_tiles<8, ERR_ROUND>;
    if (a.nt)
        hipLaunchKernelGGL(tiles, dim3(a.wgs), dim3(TP_THREADS), 0, st, d_el, a.off, a.cap, a.tbase, nblocks, d_n, e.d_ref,
                           (const u64 *)a.extra[1], (const u64 *)a.extra[0], (u64 *)a.scratch, a.nt, a.per_wg);
    const u32 bw = (u32)nblocks < TP_MAX_BLOCK_WGS ? (u32)nblocks : TP_MAX_BLOCK_WGS;
    hipLaunchKernelGGL(planes_error_blocks, dim3(bw), dim3(TP_THREADS), 0, st, a.cap, a.tbase, nblocks, d_n, (const u64 *)a.scratch,
                       d_stat, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
