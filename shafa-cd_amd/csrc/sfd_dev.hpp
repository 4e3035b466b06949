// sfd_dev.hpp — Module D from DEVICE-resident code tables, block sizes and symbol counts (shafa_hipd_sf_decode_dev)
// Part of sf_decode.hip's translation unit (included there, after sfdec_launch; not compiled on its own).
//
// sfd_plan_dev (one workgroup per block) does on the device what sfdec_launch + build_host_tab + spec_worthwhile do on the
// host: it validates the table, builds the look-up tables and the trie into the block's workspace slot, runs the
// speculation verdict (spec_trial) and writes the block's DecBlk into one of four lists (empty records, n_tiles = 0, in the others):
//   p12      complete codes of <= 12 bits                   sfdec_launch's packed form (sfd_sync16<true, false> ...)
//   packed   complete codes of 13..16 bits                  the long_all form of sfdec_launch (sfd_sync16<false, true> ...)
//   bytemap  everything else of <= 32 bits                  the byte-map kernels at R = 32
//   big      codes of 33..64 bits (one block a launch)       the byte-map kernels at R = 64, one slot of max h_in_cap
// The host launches every list over all its slots with sfdec_launch's chain launchers (sfd_launch_packed, sfd_launch_bytemap),
// grids from nblocks and the capacities; tile_base comes from the capacities, so no launch parameter depends on what the
// tables hold.
#pragma once

namespace {

constexpr int SDV_TRIE_PAIRS = 8192;               // internal nodes of a code of <= 32 bits: 1 + 256 * 31 < 8192
constexpr int SDV_BIG_PAIRS = 16384;               // ... of <= 64 bits: 1 + 256 * 63
constexpr int SDV_R_BIG = 64;                       // sfdec_launch's R for codes of 33..64 bits
constexpr size_t SDV_O_LUT = 0;                                        // u16 x 2^LUT_MAXK
constexpr size_t SDV_O_LUT2 = SDV_O_LUT + (2u << LUT_MAXK);            // u16 x LUT2_MAX (+ pad)
constexpr size_t SDV_O_LEN = SDV_O_LUT2 + LUT2_MAX * 2 + 16;           // u8 x 2^LEN_MAXK + 4
constexpr size_t SDV_O_L13 = SDV_O_LEN + (1u << LEN_MAXK) + 16;        // u16 x 2^LEN_MAXK + 2
constexpr size_t SDV_O_LONG = SDV_O_L13 + (2u << LEN_MAXK) + 16;       // LONG_BYTES
constexpr size_t SDV_O_TRIE = (SDV_O_LONG + LONG_BYTES + 15) & ~(size_t)15;
constexpr size_t SDV_SLOT = SDV_O_TRIE + (size_t)SDV_TRIE_PAIRS * 8;   // per block
constexpr size_t SDV_TABS = (2u << LEN_MAXK) + (4u << LEN_MAXK) + 16384 + 2048 + (2u << LEN_MAXK);   // cnt3, sym3, fsm4, fsm1, pairlut

struct SdvHost {            // what only the host knows: per block, from its arguments
    const u8 *in;
    u8 *out;
    u64 in_cap;
    u64 out_cap;
    u32 tile_base;
    u32 pad;
};

struct SdvOut {
    DecBlk *p12, *packed, *bytemap, *big;   // lists: nblocks, nblocks, nblocks, 1 record(s)
    u8 *slots;                         // SDV_SLOT per block
    u8 *tabs;                          // SDV_TABS per block
    u32 *big_trie;                     // SDV_BIG_PAIRS pairs
    u32 *run_dp;                       // nblocks words, or NULL (no speculation)
    int speculate, path;               // the knobs of sfdec_launch
};

__device__ __forceinline__ int sdv_cmp(const u64 *a, u32 la, const u64 *b, u32 lb)
{
    for (int k = 0; k < 4; ++k)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

__global__ __launch_bounds__(256) void sfd_plan_dev(const SdvHost *__restrict__ hb, int nblocks, const u64 *__restrict__ d_in_n,
                                                    const shafa_code_table *__restrict__ tabs, const u64 *__restrict__ d_nsym,
                                                    int *__restrict__ d_err, SdvOut po)
{
    __shared__ u64 code[256][4];             // code bits, MSB first, masked to the length
    __shared__ u32 len[256], order[256], lcp[256], excl[256], grp[256], g2[256];
    __shared__ u8 raw[256][2];
    __shared__ __attribute__((aligned(16))) u16 lut[1u << LUT_MAXK];
    __shared__ __attribute__((aligned(16))) u16 lut2[LUT2_MAX];
    __shared__ __attribute__((aligned(16))) u8 lenlut[(1u << LEN_MAXK) + 16];
    __shared__ __attribute__((aligned(16))) u8 symlut[1u << LEN_MAXK];
    __shared__ __attribute__((aligned(16))) u16 longtab[LONG_BYTES / 2];
    __shared__ u64 rnd[SPEC_TRIALS * SPEC_WORDS];
    __shared__ u32 s_lmax, s_n, s_bad, s_kraft, s_fails, s_n13, s_nl2, s_ngrp, s_nodes, s_big_taken;

    const int b = blockIdx.x, tid = threadIdx.x;
    const SdvHost h = hb[b];
    const u64 in_n = d_in_n[b], nsym = d_nsym[b];
    const shafa_code_table &t = tabs[b];
    DecBlk e;
    memset(&e, 0, sizeof(e));
    e.in = h.in;
    e.out = h.out;
    e.err = d_err + b;
    e.tile_base = h.tile_base;
    if (tid == 0) { po.p12[b] = e; po.packed[b] = e; po.bytemap[b] = e; }     // empty records: n_tiles = 0, n_sym = 0 (sfd_offsets)
    e.in_n = in_n;
    e.n_sym = nsym;
    if (po.run_dp && tid == 0) po.run_dp[b] = 1u;
    if (in_n > h.in_cap || nsym > h.out_cap) {
        if (tid == 0) set_error(e.err, SHAFA_OUTSIDE_MODULE);
        return;
    }
    if (!nsym) return;

    // ---- the codes, the longest, the prefix check (rank sort + adjacent pairs) --------------------------------------
    if (tid == 0) { s_lmax = 0; s_n = 0; s_bad = 0; s_kraft = 0; s_fails = 0; s_n13 = 0; s_big_taken = 0; }
    __syncthreads();
    const u32 L = t.len[tid];
    {
        u64 w[4] = {0, 0, 0, 0};
        for (u32 q = 0; q < (L + 7) / 8; ++q) w[q >> 3] |= (u64)t.bits[tid][q] << (56 - 8 * (q & 7));
        for (int k = 0; k < 4; ++k) {                   // bits past the length are not part of the code
            const int keep = (int)L - 64 * k;
            if (keep <= 0) w[k] = 0;
            else if (keep < 64) w[k] &= ~0ull << (64 - keep);
            code[tid][k] = w[k];
        }
        len[tid] = L;
        raw[tid][0] = L ? t.bits[tid][0] : 0;
        raw[tid][1] = L > 8 ? t.bits[tid][1] : 0;
        if (L) { atomicMax(&s_lmax, L); atomicAdd(&s_n, 1u); }
        if (L == 13) atomicAdd(&s_n13, 1u);
    }
    __syncthreads();
    const u32 lmax = s_lmax, n = s_n;
    if (lmax == 0 || in_n == 0) {                       // empty table (or single symbol of no bits), or no stream
        if (tid == 0) set_error(e.err, SHAFA_FILE_UNRECOGNIZABLE);
        return;
    }
    if (L) {
        u32 r = 0;
        for (int s = 0; s < 256; ++s) {
            if (!len[s]) continue;
            const int c = sdv_cmp(code[s], len[s], code[tid], L);
            r += c < 0 || (c == 0 && s < tid);
        }
        order[r] = (u32)tid;
    }
    __syncthreads();
    if ((u32)tid < n) {
        const u32 s = order[tid];
        u32 l = 0;
        if (tid > 0) {
            const u32 p = order[tid - 1];
            u32 pos = 256;
            for (int k = 0; k < 4; ++k) {
                const u64 x = code[p][k] ^ code[s][k];
                if (x) { pos = 64 * k + (u32)__builtin_clzll(x); break; }
            }
            const u32 m = len[p] < len[s] ? len[p] : len[s];
            if (pos >= m) s_bad = 1;                    // duplicate, or the shorter code is a prefix of the longer one
            l = pos < m ? pos : m;
        }
        lcp[tid] = l;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) set_error(e.err, SHAFA_FILE_UNRECOGNIZABLE);
        return;
    }
    // codes of 33..64 bits: one block a launch has the R = 64 slot, the first by index that passes the checks above the
    // prefix check (symbols to decode, sizes within the capacities, a stream, a longest code of 33..64 bits); longer codes
    // have no slot.  The rule is stated in include/shafa_hip.h.
    const bool big = lmax > 32;
    if (lmax > (u32)SDV_R_BIG) {
        if (tid == 0) set_error(e.err, SHAFA_LACK_OF_MEMORY);
        return;
    }
    if (big) {
        for (int q = tid; q < b; q += 256) {
            const u64 qs = d_nsym[q], qn = d_in_n[q];
            if (!qs || !qn || qn > hb[q].in_cap || qs > hb[q].out_cap) continue;
            u32 m = 0;
            for (int s = 0; s < 256; ++s) m = tabs[q].len[s] > m ? tabs[q].len[s] : m;
            if (m > 32 && m <= (u32)SDV_R_BIG) s_big_taken = 1;
        }
        __syncthreads();
        if (s_big_taken) {
            if (tid == 0) set_error(e.err, SHAFA_LACK_OF_MEMORY);
            return;
        }
    }

    // ---- the trie: in sorted order, code i adds the internal nodes at depths lcp_i + 1 .. L_i - 1 ---------------------
    if (tid == 0) {
        u32 acc = 0;
        for (u32 i = 0; i < n; ++i) { excl[i] = acc; acc += len[order[i]] - 1 - lcp[i]; }
        s_nodes = 1 + acc;
    }
    __syncthreads();
    u8 *slot = po.slots + (size_t)b * SDV_SLOT;
    u32 *trie = big ? po.big_trie : (u32 *)(slot + SDV_O_TRIE);
    const u32 nodes = s_nodes;
    for (u32 i = tid; i < 2 * nodes; i += 256) trie[i] = 0xFFFFFFFFu;
    __syncthreads();
    if ((u32)tid < n) {
        const u32 i = (u32)tid, s = order[i], Ls = len[s], l0 = lcp[i];
        auto id = [&](u32 j, u32 d) { return 1u + excl[j] + (d - lcp[j] - 1u); };
        u32 parent = 0;
        if (l0) {                                        // the node at depth l0 was made by the last code before with lcp < l0
            u32 j = i - 1;
            while (j > 0 && lcp[j] >= l0) --j;
            parent = id(j, l0);
        }
        for (u32 d = l0; d < Ls; ++d) {
            const u32 bit = (u32)(code[s][d >> 6] >> (63 - (d & 63))) & 1u;
            const u32 child = d + 1 == Ls ? (0x80000000u | s) : id(i, d + 1);
            trie[2 * parent + bit] = child;
            parent = child;
        }
    }

    // ---- lut (K bits), lenlut / symlut (K1 bits), Kraft sum ---------------------------------------------------------
    const u32 K = lmax < (u32)LUT_MAXK ? lmax : (u32)LUT_MAXK;
    const u32 K1 = lmax < (u32)LEN_MAXK ? lmax : (u32)LEN_MAXK;
    for (u32 i = tid; i < (1u << LUT_MAXK); i += 256) lut[i] = 0;
    for (u32 i = tid; i < LUT2_MAX; i += 256) lut2[i] = 0;
    for (u32 i = tid; i < (1u << LEN_MAXK) + 16; i += 256) lenlut[i] = 0;
    for (u32 i = tid; i < LONG_BYTES / 2; i += 256) longtab[i] = 0;
    __syncthreads();
    const u32 c32 = L ? (u32)(code[tid][0] >> 32) >> (L < 32 ? 32 - L : 0) : 0u;     // first min(L, 32) bits, right-aligned
    if (L && L <= K)
        for (u32 i = 0, lo = c32 << (K - L); i < (1u << (K - L)); ++i) lut[lo + i] = (u16)(tid | (L << 8));
    if (L && L <= K1)
        for (u32 i = 0, lo = c32 << (K1 - L); i < (1u << (K1 - L)); ++i) { lenlut[lo + i] = (u8)L; symlut[lo + i] = (u8)tid; }
    if (L && lmax <= 16) atomicAdd(&s_kraft, 1u << (16 - L));
    __syncthreads();
    bool packed = po.path == 0 && lmax <= 16 && s_kraft == 65536u;

    // ---- 13..16-bit codes grouped by their first 12 bits (packed blocks with codes of more than 12 bits) ------------
    if (tid == 0) {
        s_ngrp = 0;
        if (packed && lmax > (u32)SYM3_MAXK) {
            u32 ng = 0, last = 0xFFFFFFFFu;
            for (u32 i = 0; i < n; ++i) {
                const u32 s = order[i], Ls = len[s];
                if (Ls <= (u32)SYM3_MAXK) continue;
                const u32 key = (u32)(code[s][0] >> (64 - SYM3_MAXK));
                if (key != last) {
                    if (ng < (u32)LONG_PFX) longtab[8 + ng] = (u16)key;
                    ++ng;
                    last = key;
                }
                grp[s] = ng - 1;
            }
            s_ngrp = ng;
            longtab[0] = (u16)ng;
        }
    }
    __syncthreads();
    if (s_ngrp > (u32)LONG_PFX) packed = false;         // (uniform)
    if (packed && lmax > (u32)SYM3_MAXK && L > (u32)SYM3_MAXK) {
        const u32 suf = (c32 & ((1u << (L - SYM3_MAXK)) - 1)) << (16 - L);
        for (u32 i = 0; i < (1u << (16 - L)); ++i) longtab[8 + LONG_PFX + grp[tid] * 16 + suf + i] = (u16)(tid | (L << 8));
    }

    // ---- level 2: the codes of K+1..K+8 bits grouped by their first K bits (sorted order: a group is contiguous) -------
    if (tid == 0) {
        u32 base = 0;
        for (u32 i = 0; i < n;) {
            const u32 s = order[i], Ls = len[s];
            g2[s] = 0xFFFFFFFFu;
            if (Ls <= K || Ls > K + 8) { ++i; continue; }
            const u32 pre = (u32)(code[s][0] >> (64 - K));
            u32 j = i, maxl = 0;
            for (; j < n && (u32)(code[order[j]][0] >> (64 - K)) == pre; ++j) {
                const u32 l2 = len[order[j]];
                g2[order[j]] = 0xFFFFFFFFu;
                if (l2 > K && l2 <= K + 8 && l2 > maxl) maxl = l2;
            }
            const u32 nb = maxl - K;
            if (base + (1u << nb) <= (u32)LUT2_MAX) {
                for (u32 q = i; q < j; ++q) {
                    const u32 l2 = len[order[q]];
                    if (l2 > K && l2 <= K + 8) g2[order[q]] = base | (nb << 16);
                }
                lut[pre] = (u16)(0x8000u | ((nb - 1) << 12) | base);
                base += 1u << nb;
            }
            i = j;
        }
        s_nl2 = (base + 1) & ~1u;
    }
    __syncthreads();
    if (L > K && L <= K + 8 && g2[tid] != 0xFFFFFFFFu) {
        const u32 base = g2[tid] & 0xFFFFu, nb = g2[tid] >> 16;
        const u32 pre_bits = (u32)(code[tid][0] >> (64 - L));            // L <= 19
        const u32 sub = pre_bits & ((1u << (L - K)) - 1);
        for (u32 i = 0, lo = sub << (K + nb - L); i < (1u << (K + nb - L)); ++i) lut2[base + lo + i] = (u16)(tid | (L << 8));
    }

    // ---- the speculation verdict (spec_worthwhile's key, random bits and rule: sfd_common.hpp) ------------------------
    bool spec = false;
    if (packed && po.run_dp && lmax >= 2) {
        if (po.speculate == 2) spec = true;
        else {
            if (tid == 0) {                             // raw holds every byte of a code of <= 16 bits
                u64 rs = spec_key(len, raw) | 1ull;
                for (int i = 0; i < SPEC_TRIALS * SPEC_WORDS; ++i) rnd[i] = spec_rand(rs);
            }
            __syncthreads();
            if (tid < SPEC_TRIALS && !spec_trial(rnd + SPEC_WORDS * tid, lenlut, K1)) atomicAdd(&s_fails, 1u);
            __syncthreads();
            spec = s_fails <= (u32)SPEC_MAX_FAILS;
        }
    }
    __syncthreads();

    // ---- the tables into the block's slot, the record into its list -------------------------------------------------
    u16 *g_lut = (u16 *)(slot + SDV_O_LUT), *g_lut2 = (u16 *)(slot + SDV_O_LUT2), *g_l13 = (u16 *)(slot + SDV_O_L13);
    u8 *g_len = slot + SDV_O_LEN;
    u16 *g_long = (u16 *)(slot + SDV_O_LONG);
    for (u32 i = tid; i < (1u << K); i += 256) g_lut[i] = lut[i];
    for (u32 i = tid; i < s_nl2; i += 256) g_lut2[i] = lut2[i];
    for (u32 i = tid; i < (1u << K1) + 4; i += 256) g_len[i] = lenlut[i];
    for (u32 i = tid; i < (1u << K1) + 2; i += 256)
        g_l13[i] = i < (1u << K1) && lenlut[i] ? (u16)(symlut[i] | ((u32)lenlut[i] << 8)) : (u16)0;
    const bool has_long = packed && lmax > (u32)SYM3_MAXK;
    if (has_long)
        for (u32 i = tid; i < LONG_BYTES / 2; i += 256) g_long[i] = longtab[i];
    if (tid) return;
    e.lut = g_lut;
    e.lut2 = g_lut2;
    e.n_l2 = s_nl2;
    e.lenlut = g_len;
    e.lenlut32 = g_len;
    e.lut13 = g_l13;
    e.trie = trie;
    e.K = K;
    e.K1 = K1;
    e.lmax = lmax;
    e.n_states = nodes;
    e.n_tiles = (u32)((in_n + DTILE - 1) / DTILE);
    e.one = 0;                                          // (the launch's kernels are chosen before the tables are known)
    if (packed) {
        u8 *tb = po.tabs + (size_t)b * SDV_TABS;
        e.cnt3 = (u16 *)tb;
        e.sym3 = (u32 *)(tb + (2u << LEN_MAXK));
        e.fsm4 = (u32 *)(tb + (6u << LEN_MAXK));
        e.fsm1 = (u32 *)(tb + (6u << LEN_MAXK) + 16384);
        e.longtab = has_long ? g_long : nullptr;
        e.run_dp = po.run_dp ? po.run_dp + b : nullptr;
        if (po.run_dp) po.run_dp[b] = spec ? 0u : 1u;
        if (lmax <= (u32)SYM3_MAXK) {                  // every window of K1 bits starts a code: the pair table
            e.pairlut = tb + (6u << LEN_MAXK) + 16384 + 2048;
            e.KW = spec_window(K1);
            po.p12[b] = e;
        } else {
            e.KW = scan_window(K1, true, s_n13);          // with the table of long codes, as sfdec_launch's long_all form
            po.packed[b] = e;
        }
    } else if (big) {
        e.tile_base = 0;                               // the big slot's own tile arrays
        *po.big = e;
    } else po.bytemap[b] = e;
}

}  // namespace

int sfdec_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, const shafa_code_table *d_tables, const u64 *d_n_symbols, u8 *d_out,
                     const u64 *h_out_off, const u64 *h_out_cap)
{
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    u64 total = 0;
    u32 max_tiles = 0;
    for (int b = 0; b < nblocks; ++b) {
        if ((h_in_off[b] & 15) || (h_out_off[b] & 15)) return SHAFA_OUTSIDE_MODULE;
        const u64 t = ceil_div_u64(h_in_cap[b], DTILE);
        total += t;
        if (t > max_tiles) max_tiles = (u32)t;
    }
    if (total >= 0xFFFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    const size_t T = (size_t)total, MT = max_tiles;
    const bool spec = g_sfd_speculate != 0;
    constexpr u32 R = 32;

    // workspace: lists | run_dp | slots | packed tables | big trie | per-tile arrays (capacity tiles) | the big slot's own
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    const size_t o_l12 = take((size_t)nblocks * sizeof(DecBlk)), o_lp = take((size_t)nblocks * sizeof(DecBlk)), o_lb = take((size_t)nblocks * sizeof(DecBlk)),
                 o_lg = take(sizeof(DecBlk)), o_rundp = take((size_t)nblocks * 4), o_slot = take((size_t)nblocks * SDV_SLOT),
                 o_tabs = take((size_t)nblocks * SDV_TABS), o_btrie = take((size_t)SDV_BIG_PAIRS * 8);
    const size_t o_tent = take(T), o_tcnt = take(T * 4), o_toff = take(T * 8), o_cent = take(T * DEC_THREADS),
                 o_ccnt = take(T * DEC_THREADS * 2), o_tguess = take(spec ? T : 0), o_texit = take(spec ? T : 0);
    const size_t o_pcfn = take(T * DEC_THREADS * 8), o_ptfn = take(T * 16);                 // packed
    const size_t o_bcfn = take(T * R * DEC_THREADS), o_btfn = take(T * R);                  // bytemap
    const size_t o_gcfn = take(MT * SDV_R_BIG * DEC_THREADS), o_gtfn = take(MT * SDV_R_BIG), o_gtent = take(MT),
                 o_gtcnt = take(MT * 4), o_gtoff = take(MT * 8), o_gcent = take(MT * DEC_THREADS),
                 o_gccnt = take(MT * DEC_THREADS * 2);
    int rc = batch_reserve(bt, st, off);
    if (rc) return rc;
    u8 *ws = (u8 *)bt->d_ws;

    const size_t stage_bytes = (size_t)nblocks * sizeof(SdvHost);
    u8 *dpar = batch_params_begin(bt, stage_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    SdvHost *hp = (SdvHost *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, stage_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    u32 tbase = 0;
    for (int b = 0; b < nblocks; ++b) {
        hp[b].in = d_in + h_in_off[b];
        hp[b].out = d_out + h_out_off[b];
        hp[b].in_cap = h_in_cap[b];
        hp[b].out_cap = h_out_cap[b];
        hp[b].tile_base = tbase;
        hp[b].pad = 0;
        tbase += (u32)ceil_div_u64(h_in_cap[b], DTILE);
    }
    HIP_TRY(hipMemsetAsync(ws + o_lg, 0, sizeof(DecBlk), st));      // the big slot stays empty unless a block takes it
    if ((rc = batch_params_commit(bt, st, hp, stage_bytes))) return rc;

    SdvOut po;
    po.p12 = (DecBlk *)(ws + o_l12);
    po.packed = (DecBlk *)(ws + o_lp);
    po.bytemap = (DecBlk *)(ws + o_lb);
    po.big = (DecBlk *)(ws + o_lg);
    po.slots = ws + o_slot;
    po.tabs = ws + o_tabs;
    po.big_trie = (u32 *)(ws + o_btrie);
    po.run_dp = spec ? (u32 *)(ws + o_rundp) : nullptr;
    po.speculate = g_sfd_speculate;
    po.path = g_sfd_path;
    hipLaunchKernelGGL(sfd_plan_dev, dim3((u32)nblocks), dim3(256), 0, st, (const SdvHost *)dpar, nblocks, d_in_n, d_tables,
                       d_n_symbols, bt->d_err, po);
    if (!max_tiles) { HIP_TRY(hipGetLastError()); return pscope.done(); }

    // ---- packed lists: <= 12 bits in sfdec_launch's packed form (pair table, no escapes), 13..16 bits in its long_all form
    // (the whole table of long codes in LDS).  Both share the per-tile arrays: a block is in one list only.  The symbol image
    // is fixed, for four workgroups per CU (a tile that exceeds it goes in rounds); sfdec_launch gives 12-bit tables on Zipf
    // data the same 40 KiB.
    const SfdArrays pa = {ws + o_pcfn, ws + o_ptfn, ws + o_tent, ws + o_cent, (u16 *)(ws + o_ccnt), (u32 *)(ws + o_tcnt),
                          (u64 *)(ws + o_toff), ws + o_tguess, ws + o_texit};
    for (const bool lng : {false, true}) {
        const u32 long_used = lng ? (u32)LONG_BYTES : 0u;   // the table of any block (header, prefixes, 128 groups)
        const u32 ws_tab = 4u << SYM3_MAXK;
        const u32 ws_cap = (40960u - (u32)ws_rows_bytes(lng) - ws_tab - long_used - (u32)WS_MISC) & ~15u;
        sfd_launch_packed(st, lng ? po.packed : po.p12, nblocks, max_tiles, lng ? SFD_LONG_ALL : SFD_PACKED, lng, spec,
                          2u << (lng ? LEN_MAXK : SYM3_MAXK), long_used, false, ws_tab, ws_cap, pa);
    }
    // ---- byte-map lists: R = 32 over every slot, R = 64 over the one big slot ---------------------------------------
    const u32 l2cap = (u32)LUT2_MAX + 8;
    const SfdArrays ba = {ws + o_bcfn, ws + o_btfn, ws + o_tent, ws + o_cent, (u16 *)(ws + o_ccnt), (u32 *)(ws + o_tcnt),
                          (u64 *)(ws + o_toff), nullptr, nullptr};
    const SfdArrays ga = {ws + o_gcfn, ws + o_gtfn, ws + o_gtent, ws + o_gcent, (u16 *)(ws + o_gccnt), (u32 *)(ws + o_gtcnt),
                          (u64 *)(ws + o_gtoff), nullptr, nullptr};
    if ((rc = sfd_launch_bytemap(st, po.bytemap, (u32)nblocks, max_tiles, R, l2cap, ba))) return rc;
    if ((rc = sfd_launch_bytemap(st, po.big, 1u, max_tiles, SDV_R_BIG, l2cap, ga))) return rc;
    HIP_TRY(hipGetLastError());
    return pscope.done();
}
