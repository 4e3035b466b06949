// planes_arith.hpp — what planes.hip (the plain, XOR and difference transposes) and planes_lag.hip (the lagged differences)
// share: the unit of 16 elements a lane and its transposition in registers (pick4, split_dword, merge_dword, split_store), the
// arithmetic on element-ordered dwords (SWAR at 1 and 2 bytes: pk_*, the zigzag fold, the sums and scans), the element side's
// aligned words shifted into place (load_words, shift_into) and the workgroup's exclusive scan (wg_excl_scan).
#pragma once

#include "common.hpp"
#include "internal.hpp"
#include "tile_pass.hpp"

namespace {

constexpr int PL_UNIT = 16;                                     // elements a lane transposes at a time
constexpr int PL_PASS = TP_THREADS * PL_UNIT;                   // elements the workgroup covers with one unit a lane
constexpr int PL_UNITS = TP_TILE / PL_PASS;
static_assert(TP_TILE == SHAFA_PLANES_TILE && PL_UNITS * PL_PASS == TP_TILE, "the tile the header names");

// bytes s0 .. s3 (byte s & 3 of dword s >> 2) of w as one dword, low byte first.  The positions are constants once the
// callers' loops are unrolled: one v_perm_b32 when two dwords hold the four bytes, else three.
__device__ __forceinline__ u32 pick4(const u32 *w, int s0, int s1, int s2, int s3)
{
    const int d[4] = {s0 >> 2, s1 >> 2, s2 >> 2, s3 >> 2};
    const u32 by[4] = {(u32)s0 & 3u, (u32)s1 & 3u, (u32)s2 & 3u, (u32)s3 & 3u};
    int other = d[0];
    for (int k = 1; k < 4; ++k)
        if (d[k] != d[0]) other = d[k];
    if ((d[1] == d[0] || d[1] == other) && (d[2] == d[0] || d[2] == other)) {
        u32 sel = 0;
        for (int k = 0; k < 4; ++k) sel |= (d[k] == d[0] ? by[k] : 4u + by[k]) << (8 * k);
        return __builtin_amdgcn_perm(w[other], w[d[0]], sel);  // selector 0..3: the second operand's bytes, 4..7: the first's
    }
    const u32 lo = __builtin_amdgcn_perm(w[d[1]], w[d[0]], by[0] | (4u + by[1]) << 8);
    const u32 hi = __builtin_amdgcn_perm(w[d[3]], w[d[2]], by[2] | (4u + by[3]) << 8);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// dword q of plane j of the 16 elements in w
template <int E>
__device__ __forceinline__ u32 split_dword(const u32 (&w)[4 * E], int j, int q)
{
    return pick4(w, (4 * q) * E + j, (4 * q + 1) * E + j, (4 * q + 2) * E + j, (4 * q + 3) * E + j);
}

// dword d of the 16 elements whose plane j is p[4 j .. 4 j + 3]: byte s of the elements is byte s / E of plane s % E
template <int E>
__device__ __forceinline__ u32 merge_dword(const u32 (&p)[4 * E], int d)
{
    int s[4];
    for (int k = 0; k < 4; ++k) s[k] = 16 * ((4 * d + k) % E) + (4 * d + k) / E;
    return pick4(p, s[0], s[1], s[2], s[3]);
}

// ---- differences: the arithmetic on element-ordered dwords, E bytes an element.  At E = 1 and 2 a dword holds 4 or 2 elements
// and the operations are SWAR (H: every element's top bit, L: its low bit); sums are carried in DiffT<E>, whose low 8 E bits count.
template <int E> struct DiffT { using T = u32; };
template <> struct DiffT<8> { using T = u64; };
template <int E> __device__ __forceinline__ constexpr u32 pk_h() { return E == 1 ? 0x80808080u : 0x80008000u; }
template <int E> __device__ __forceinline__ constexpr u32 pk_l() { return E == 1 ? 0x01010101u : 0x00010001u; }
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
typedef short i16x2_t __attribute__((ext_vector_type(2)));
template <int E> __device__ __forceinline__ u32 pk_add(u32 a, u32 b)
{
    if (E == 2) return __builtin_bit_cast(u32, __builtin_bit_cast(u16x2_t, a) + __builtin_bit_cast(u16x2_t, b));     // v_pk_add_u16
    return ((a & ~pk_h<E>()) + (b & ~pk_h<E>())) ^ ((a ^ b) & pk_h<E>());
}
template <int E> __device__ __forceinline__ u32 pk_sub(u32 a, u32 b)
{
    if (E == 2) return __builtin_bit_cast(u32, __builtin_bit_cast(u16x2_t, a) - __builtin_bit_cast(u16x2_t, b));     // v_pk_sub_u16
    return ((a | pk_h<E>()) - (b & ~pk_h<E>())) ^ ((a ^ ~b) & pk_h<E>());
}
// c in every element of a dword; all ones in every element whose low bit is set in m (m has no other bit)
template <int E> __device__ __forceinline__ u32 pk_all(u32 c) { return (c & (E == 1 ? 0xFFu : 0xFFFFu)) * pk_l<E>(); }
template <int E> __device__ __forceinline__ u32 pk_ones(u32 m) { return m * (E == 1 ? 0xFFu : 0xFFFFu); }

// z = (d << 1) XOR (all ones where d's top bit is set), and its inverse, on every element of the N dwords w
template <int E, int N>
__device__ __forceinline__ void zz_fold(u32 *w)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (E == 8) {
            if (i & 1) {
                const u64 d = (u64)w[i] << 32 | w[i - 1], z = (d << 1) ^ (u64)((long long)d >> 63);
                w[i - 1] = (u32)z; w[i] = (u32)(z >> 32);
            }
        } else if (E == 4) w[i] = (w[i] << 1) ^ (u32)((int)w[i] >> 31);
        else if (E == 2) {
            const u16x2_t d = __builtin_bit_cast(u16x2_t, w[i]);
            const i16x2_t m = __builtin_bit_cast(i16x2_t, w[i]) >> (i16x2_t)(15);
            w[i] = __builtin_bit_cast(u32, (u16x2_t)(d << (u16x2_t)(1))) ^ __builtin_bit_cast(u32, m);
        } else w[i] = ((w[i] & ~pk_h<E>()) << 1) ^ pk_ones<E>((w[i] >> (8 * E - 1)) & pk_l<E>());
    }
}
template <int E, int N>
__device__ __forceinline__ void zz_unfold(u32 *w)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (E == 8) {
            if (i & 1) {
                const u64 z = (u64)w[i] << 32 | w[i - 1], d = (z >> 1) ^ (0ull - (z & 1ull));
                w[i - 1] = (u32)d; w[i] = (u32)(d >> 32);
            }
        } else if (E == 4) w[i] = (w[i] >> 1) ^ (0u - (w[i] & 1u));
        else w[i] = ((w[i] >> 1) & ~pk_h<E>()) ^ pk_ones<E>(w[i] & pk_l<E>());
    }
}

// the elements of the 16 in w -> the fold of their difference to the element in front, prev in front of the first
template <int E>
__device__ __forceinline__ void diff_fold(u32 (&w)[4 * E], typename DiffT<E>::T prev)
{
    if (E == 8) {
        u64 p = prev;
#pragma unroll
        for (int i = 0; i < 4 * E; i += 2) {
            const u64 x = (u64)w[i + 1] << 32 | w[i], d = x - p;
            p = x;
            w[i] = (u32)d; w[i + 1] = (u32)(d >> 32);
        }
    } else if (E == 4) {
        u32 p = (u32)prev;
#pragma unroll
        for (int i = 0; i < 4 * E; ++i) {
            const u32 x = w[i];
            w[i] = x - p;
            p = x;
        }
    } else {
        u32 pv = (u32)prev << (32 - 8 * E);          // the dword in front: its last element is what counts
#pragma unroll
        for (int i = 0; i < 4 * E; ++i) {
            const u32 x = w[i];
            const u32 sh = E == 1 ? __builtin_amdgcn_alignbyte(x, pv, 3) : __builtin_amdgcn_alignbit(x, pv, 16);
            pv = x;
            w[i] = pk_sub<E>(x, sh);                 // every element minus the one in front of it
        }
    }
    zz_fold<E, 4 * E>(w);
}

// the inclusive prefix sums of the elements of the N dwords w, in place; returns the last one, their total
template <int E, int N>
__device__ __forceinline__ typename DiffT<E>::T scan_incl(u32 *w)
{
    if (E == 8) {
        u64 acc = 0;
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            acc += (u64)w[i + 1] << 32 | w[i];
            w[i] = (u32)acc; w[i + 1] = (u32)(acc >> 32);
        }
        return (typename DiffT<E>::T)acc;
    } else if (E == 4) {
#pragma unroll
        for (int i = 1; i < N; ++i) w[i] += w[i - 1];
        return w[N - 1];
    } else {
        u32 carry = 0;                               // the total so far, in every element
#pragma unroll
        for (int i = 0; i < N; ++i) {
            u32 v = w[i];
            v = pk_add<E>(v, v << (8 * E));
            if (E == 1) v = pk_add<E>(v, v << 16);
            v = pk_add<E>(v, carry);
            w[i] = v;
            carry = pk_all<E>(v >> (32 - 8 * E));
        }
        return w[N - 1] >> (32 - 8 * E);
    }
}

// c onto every element of the N dwords w
template <int E, int N>
__device__ __forceinline__ void add_all(u32 *w, typename DiffT<E>::T c)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (E == 8) {
            if (i & 1) {
                const u64 v = ((u64)w[i] << 32 | w[i - 1]) + c;
                w[i - 1] = (u32)v; w[i] = (u32)(v >> 32);
            }
        } else if (E == 4) w[i] += (u32)c;
        else w[i] = pk_add<E>(w[i], pk_all<E>((u32)c));
    }
}

// the sum of the elements of the N dwords w
template <int E, int N>
__device__ __forceinline__ typename DiffT<E>::T sum_of(const u32 *w)
{
    typename DiffT<E>::T s = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (E == 8) {
            if (i & 1) s += (u64)w[i] << 32 | w[i - 1];
        } else if (E == 4) s += w[i];
        else if (E == 2) s += (w[i] & 0xFFFFu) + (w[i] >> 16);
        else s = __builtin_amdgcn_udot4(w[i], 0x01010101u, (u32)s, false);
    }
    return s;
}

// element e - 1 of the region at src, any alignment: single bytes (one lane a wave asks)
template <int E>
__device__ __forceinline__ typename DiffT<E>::T elem_in_front(const u8 *src, u64 e)
{
    typename DiffT<E>::T v = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) v |= (typename DiffT<E>::T)gload<u8>(src + (e - 1) * E + k) << (8 * k);
    return v;
}

// the element in front of a lane's unit w once every lane of the wave in front of it holds its own unit: the last element of
// the lane in front, and own0 (loaded by the caller, elem_in_front) for the wave's first lane
template <int E>
__device__ __forceinline__ typename DiffT<E>::T prev_of(const u32 (&w)[4 * E], typename DiffT<E>::T own0)
{
    typename DiffT<E>::T up;
    if (E == 8) up = (u64)(u32)__shfl_up((int)w[4 * E - 1], 1, 64) << 32 | (u32)__shfl_up((int)w[4 * E - 2], 1, 64);
    else up = (u32)__shfl_up((int)w[4 * E - 1], 1, 64) >> (32 - 8 * E);
    return lane_id() == 0 ? own0 : up;
}

// the 16 elements w from element e0 < n -> one word of each plane; single bytes where the block ends inside the unit
template <int E>
__device__ __forceinline__ void split_store(const u32 (&w)[4 * E], u64 n, u64 e0, u8 *d_planes, const u64 *poff)
{
    const u32 c = n - e0 >= PL_UNIT ? PL_UNIT : (u32)(n - e0);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const uint4 o = make_uint4(split_dword<E>(w, j, 0), split_dword<E>(w, j, 1), split_dword<E>(w, j, 2), split_dword<E>(w, j, 3));
        u8 *dst = d_planes + poff[j] + e0;
        if (c == PL_UNIT) gstore_nt<uint4>(dst, o);           // 1 KiB a wave, whole lines: streamed
        else {
#pragma unroll
            for (int k = 0; k < PL_UNIT; ++k)
                if ((u32)k < c) gstore<u8>(dst + k, tp_byte_of(o, k));
        }
    }
}

// The aligned words around bytes p .. p + 16 W - 1 (p a multiple of 16, below nbytes) of a region of nbytes bytes at src,
// src mod 16 = sh: word i is read only where it holds a byte of the region, the others are 0.  NT: streamed loads.
template <int W, bool NT>
__device__ __forceinline__ void load_words(const u8 *src, u64 nbytes, u64 p, u32 sh, uint4 (&a)[W + 1])
{
    const u8 *s16 = (const u8 *)(((u64)(uintptr_t)src + p) & ~(u64)15);
#pragma unroll
    for (int i = 0; i <= W; ++i) {
        a[i] = make_uint4(0, 0, 0, 0);
        if (i == 0 || (p + 16u * i - sh < nbytes && (i < W || sh != 0)))
            a[i] = NT ? gload_nt<uint4>(s16 + 16 * i) : gload<uint4>(s16 + 16 * i);
    }
}

// bytes 4 Q + r .. + 16 W - 1 of the words a -> the dwords w, or (XOR) onto them
template <int W, int Q, bool XOR>
__device__ __forceinline__ void shift_into(const uint4 (&a)[W + 1], u32 r, u32 *w)
{
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const uint4 v = shift_words<Q>(a[i], a[i + 1], r);
        if (XOR) { w[4 * i] ^= v.x; w[4 * i + 1] ^= v.y; w[4 * i + 2] ^= v.z; w[4 * i + 3] ^= v.w; }
        else { w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
    }
}

// The lanes' v -> their exclusive prefix sums over the workgroup, on top of carry; carry += the workgroup's total.  Every lane
// of the workgroup calls.  wt: 2 x 4 words of LDS whose halves alternate between calls (turn), so one barrier a call is enough.
template <typename T>
__device__ __forceinline__ T wg_excl_scan(T v, T &carry, T *wt, u32 &turn)
{
    T *slot = wt + 4u * (turn & 1u);
    ++turn;
    const T incl = wave_incl_scan_add<T>(v);
    if (lane_id() == 63) slot[wave_id()] = incl;
    lds_barrier();
    T pre = carry + incl - v;
#pragma unroll
    for (int q = 0; q < TP_THREADS / 64; ++q) {
        const T t = slot[q];
        if (q < wave_id()) pre += t;
        carry += t;
    }
    return pre;
}

}  // namespace
