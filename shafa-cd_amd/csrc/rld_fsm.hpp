// rld_fsm.hpp — the RLE token machine, shared by the decoder (rle_decode.hip) and the size pass (rle_measure.hip).
//
// A 0 byte may be an escape, a symbol or a count, so token boundaries are found with a 3-state machine
//     S0 (token start): b == 0 -> S1, else literal -> S0      S1 (symbol) -> S2      S2 (count) -> S0
// which only looks at "is the byte zero".  A map {S0,S1,S2} -> {S0,S1,S2} is 6 bits (2 per entry state); maps compose
// (fn_compose, associative), so any cut of a stream into pieces can be put together again in order.
#pragma once

#include "common.hpp"
#include "tile_pass.hpp"

namespace {

// the decoder's tile is the size pass's: its exact output regions are measured tile by tile
constexpr int RLD_THREADS = TP_THREADS;
constexpr int RLD_BPL = TP_BPL;                    // bytes per lane (fsm32 takes a lane's zero mask)
constexpr int RLD_TILE = TP_TILE;
constexpr u32 FN_IDENT = 0u | (1u << 2) | (2u << 4);

// per 8-bit zero mask (bit i = byte i is 0) and entry state s: bits [10 s, 10 s + 8) = token starts, [10 s + 8, 10 s + 10) = exit
struct RldFsm {
    u32 v[256];
    constexpr RldFsm() : v()
    {
        for (u32 z = 0; z < 256; ++z) {
            u32 e = 0;
            for (u32 s0 = 0; s0 < 3; ++s0) {
                u32 st = s0, starts = 0;
                for (u32 i = 0; i < 8; ++i) {
                    if (st == 0) { starts |= 1u << i; st = ((z >> i) & 1u) ? 1u : 0u; }
                    else st = st == 1 ? 2u : 0u;
                }
                e |= (starts | (st << 8)) << (10 * s0);
            }
            v[z] = e;
        }
    }
};
__device__ const RldFsm g_rld_fsm = RldFsm();

// apply a first, then b
__device__ __forceinline__ u32 fn_compose(u32 a, u32 b)
{
    const u32 r0 = (b >> (2 * (a & 3))) & 3;
    const u32 r1 = (b >> (2 * ((a >> 2) & 3))) & 3;
    const u32 r2 = (b >> (2 * ((a >> 4) & 3))) & 3;
    return r0 | (r1 << 2) | (r2 << 4);
}
__device__ __forceinline__ u32 fn_apply(u32 f, u32 s) { return (f >> (2 * s)) & 3; }
__device__ __forceinline__ bool fn_const(u32 f) { return (f & 3) == ((f >> 2) & 3) && (f & 3) == ((f >> 4) & 3); }

// zero mask of 32 bytes -> token-start mask and exit state for each of the three entry states
__device__ __forceinline__ void fsm32(const u32 *fsm, u32 z, u32 (&st3)[3], u32 (&ex3)[3])
{
    const u32 e0 = fsm[z & 255u], e1 = fsm[(z >> 8) & 255u], e2 = fsm[(z >> 16) & 255u], e3 = fsm[z >> 24];
#pragma unroll
    for (int s0 = 0; s0 < 3; ++s0) {
        u32 x = (e0 >> (10 * s0)) & 1023u, starts = x & 255u;
        x = (e1 >> (10 * (x >> 8))) & 1023u; starts |= (x & 255u) << 8;
        x = (e2 >> (10 * (x >> 8))) & 1023u; starts |= (x & 255u) << 16;
        x = (e3 >> (10 * (x >> 8))) & 1023u; starts |= (x & 255u) << 24;
        st3[s0] = starts;
        ex3[s0] = x >> 8;
    }
}

// bit i of a nibble -> 0x01 in byte i
__device__ __forceinline__ u32 nib_flags(u32 mask, int i) { return __umul24((mask >> (4 * i)) & 15u, 0x00204081u) & 0x01010101u; }

}  // namespace
