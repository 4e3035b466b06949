// unpack.hip — the inverse of pack.hip: the project's files, held in device memory, parsed into what the device decoders take
// (shafa_hipd_unpack_cod / _unpack_rle_freq / _unpack_freq / _unpack_shaf / _unpack_payloads).
//
// The rules are those of the C host (host/modules.c read_header / read_block / shaf_read_u64, host/formats.c shafa_cod_parse
// and shafa_freq_parse):
//   .cod   "@<mode>@<n>", then "@<size>@" + "c0;c1;...;c255" per block        -> sizes, binary tables
//   .freq  "@<mode>@<n>", then "@<size>@" + fields per block (framing only)   -> sizes, offsets of the payloads in the .rle
//   .freq  the same text, fields parsed (unpack_freq)                         -> sizes, 256 counts per block
//   .shaf  "@<n>", then "@<size>@" + payload per block                         -> offsets and sizes of the payloads
//
// Kernels (stable names for rocprofv3):
//   unpack_at_count       a workgroup per 4 KiB chunk of a .cod / .freq text: its '@' count
//   unpack_at_scan        ONE workgroup: exclusive scan of the chunk counts, the text's '@' total
//   unpack_at_place       a workgroup per chunk: the positions of the first 2 max_blocks + 4 '@' (inside these two files '@' only
//                         separates fields, so block b's frame is the '@' of rank k0 + 2b, k0 + 2b + 1 and k0 + 2b + 2)
//   unpack_frames         ONE workgroup looping over the blocks: the header, every block's frame as read_block checks it, the
//                         first failing block (block order), sizes, text spans, the .rle offsets, d_info
//   unpack_tables         a workgroup per block, a lane per symbol: shafa_cod_parse in LDS -> the binary table
//   unpack_counts         a workgroup per block, a lane per field: shafa_freq_parse in LDS -> the 256 counts
//   unpack_shaf_walk      ONE wave: the dependent chain of the .shaf headers, one 32-byte window per block
//   unpack_move_plan      a lane per block: the capacity and file checks, two descriptor records for pack.hip's movers
// The payloads themselves are moved by pack.hip's pack_bulk / pack_seams (pack_move_launch): no second mover.
// Segmented parses (shafa_hipd_unpack_*_files: many files in one launch sequence) add
//   unpack_at_count_files  a workgroup per (file, chunk) pair of a host-built list: at_count on that chunk
//   unpack_at_place_files  a workgroup per pair: at_place with the file's ranks (the unchanged unpack_at_scan runs over the
//                          whole list in between: a file's ranks are differences of its chunks' bases)
//   unpack_frames_files    a workgroup per file: unpack_frames' body (frames) on its text
//   unpack_shaf_walk_files a wave per file: unpack_shaf_walk's body (shaf_walk) on its .shaf
// and run unpack_tables as it is, once per run of consecutive slots.
//
// Reads: every load of a file is a byte load of a byte inside [file, file + n), except pack_bulk's and unpack_counts' aligned
// 16-byte words, each of which holds a byte of the payload it moves / of the block text it parses.  Writes: only the caller's arrays of max_blocks (nblocks) entries and d_info
// (segmented: the files' slots and their records).
#include "common.hpp"
#include "internal.hpp"

#include <algorithm>

namespace {

constexpr int IDX_THREADS = 256;
constexpr u32 IDX_BYTES = 16;                                 // text bytes per lane in the '@' count and placement
constexpr u64 IDX_CHUNK = (u64)IDX_THREADS * IDX_BYTES;      // 4 KiB of text per workgroup
constexpr int FRAME_THREADS = 256;
constexpr u32 COD_TEXT_MAX = 33151;                           // SHAFA_COD_BLOCK_MAX (host/shafa_host.h)
constexpr u32 FREQ_TEXT_MAX = 256 * 20 + 255;                 // SHAFA_FREQ_BLOCK_MAX
constexpr u32 FREQ_TEXT_WORDS = (15 + FREQ_TEXT_MAX + 15) / 16;  // 16-byte words that hold a block text at any alignment

struct TextSpan {
    u64 start;               // the block's text: [start, start + n) of the file, after its "@<size>@"
    u64 n;                   // 0: not parsed (a block after the first framing failure, or beyond the header's count)
};

// workspace of a text index: [total '@': 16 B][chunk counts: u32][chunk bases: u64][positions: u64 x limit][spans]
struct IdxWs {
    u64 *total;
    u32 *cnt;
    u64 *base;
    u64 *pos;
    TextSpan *spans;
};

__device__ inline bool is_digit(u8 c) { return c >= '0' && c <= '9'; }

// chunk c of the text: its '@' count to *out
__device__ __forceinline__ void at_count(const u8 *__restrict__ t, u64 n, u64 c, u32 *__restrict__ out)
{
    __shared__ u32 wsum[IDX_THREADS / 64];
    const u64 p0 = c * IDX_CHUNK + (u64)threadIdx.x * IDX_BYTES;
    u32 k = 0;
    for (u32 i = 0; i < IDX_BYTES; ++i)
        if (p0 + i < n && t[p0 + i] == '@') ++k;
    const u32 incl = dpp_scan_add(k);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) *out = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(IDX_THREADS) void unpack_at_count(const u8 *__restrict__ t, u64 n, u32 *__restrict__ cnt)
{
    at_count(t, n, blockIdx.x, cnt + blockIdx.x);
}

// one workgroup: base[c] = sum of cnt[0 .. c), *total = the text's '@' count
__global__ __launch_bounds__(IDX_THREADS) void unpack_at_scan(const u32 *__restrict__ cnt, u64 nchunks, u64 *__restrict__ base,
                                                              u64 *__restrict__ total)
{
    __shared__ u64 wsum[IDX_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    u64 run = 0;
    for (u64 c0 = 0; c0 < nchunks; c0 += IDX_THREADS) {
        const u64 c = c0 + tid;
        const u64 v = c < nchunks ? cnt[c] : 0;
        const u64 incl = wave_incl_scan_add<u64>(v);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        u64 before = 0, all = 0;
        for (u32 w = 0; w < IDX_THREADS / 64; ++w) {
            if (w < wv) before += wsum[w];
            all += wsum[w];
        }
        if (c < nchunks) base[c] = run + before + incl - v;
        run += all;
        __syncthreads();
    }
    if (tid == 0) *total = run;
}

// chunk c of the text, whose first '@' has rank b0: the positions of the '@' of rank < limit, in text order
__device__ __forceinline__ void at_place(const u8 *__restrict__ t, u64 n, u64 c, u64 b0, u64 limit, u64 *__restrict__ pos)
{
    __shared__ u32 wsum[IDX_THREADS / 64];
    if (b0 >= limit) return;                                     // uniform per workgroup
    const u64 p0 = c * IDX_CHUNK + (u64)threadIdx.x * IDX_BYTES;
    u32 k = 0;
    for (u32 i = 0; i < IDX_BYTES; ++i)
        if (p0 + i < n && t[p0 + i] == '@') ++k;
    const u32 incl = dpp_scan_add(k);
    const u32 wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[wv] = incl;
    __syncthreads();
    u32 before = 0;
    for (u32 w = 0; w < wv; ++w) before += wsum[w];
    u64 r = b0 + before + incl - k;
    for (u32 i = 0; i < IDX_BYTES && r < limit; ++i)
        if (p0 + i < n && t[p0 + i] == '@') pos[r++] = p0 + i;
}

__global__ __launch_bounds__(IDX_THREADS) void unpack_at_place(const u8 *__restrict__ t, u64 n, const u64 *__restrict__ base,
                                                               u64 limit, u64 *__restrict__ pos)
{
    at_place(t, n, blockIdx.x, base[blockIdx.x], limit, pos);
}

// saturating sum: associative, so it scans like an ordinary one (.rle offsets from sizes the text may make arbitrary)
__device__ inline u64 sat_add(u64 a, u64 b) { return a + b < a ? ~(u64)0 : a + b; }

__device__ inline u64 wave_incl_scan_sat(u64 v)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(v, d, 64);
        if (lane >= d) v = sat_add(v, t);
    }
    return v;
}

struct FrameArgs {
    const u8 *t;
    u64 n;
    const u64 *total;        // the text's '@' count
    const u64 *pos;          // positions of its first `limit` '@'
    u64 limit;
    int max_blocks;
    u32 field_max;           // read_block's max_payload
    u64 *info;               // SHAFA_UNPACK_INFO_WORDS words
    u64 *sizes;              // the "@<size>@" numbers
    TextSpan *spans;         // the block texts for unpack_tables / unpack_counts; nullptr for a .freq read for its framing
    u64 *off;                // .rle.freq: the payload offsets in the .rle; else nullptr
    u64 rle_n;
    int *err;
};

// "@<mode>@<digits>" (read_header, host/modules.c): the count and the position behind its digits; false: a bad header
__device__ bool read_header(const u8 *t, u64 n, u8 *mode, u64 *count, u64 *end)
{
    if (n < 2 || t[0] != '@') return false;
    *mode = t[1];
    if (n < 3 || t[2] != '@') return false;
    u64 p = 3, x = 0;
    while (p < n && is_digit(t[p])) x = x * 10 + (u64)(t[p++] - '0');          // read_u64: unbounded digits, wrapping
    if (p == 3) return false;
    *count = x;
    *end = p;
    return x <= (n - p) / 3;                                                     // every block needs "@<digit>@"
}

// the header and every block's frame of one text, by one workgroup.  Spans and .rle offsets of framed blocks are written
// span_base / off_base bytes further on (the segmented form: from the call's base pointers, not from the file's start).
__device__ __forceinline__ void frames(const FrameArgs &a, u64 span_base, u64 off_base)
{
    __shared__ u32 hdr_ok;
    __shared__ u8 mode_sh;
    __shared__ u64 count_sh, k0_sh, nidx_sh, maxsz_sh, run_sh;
    __shared__ int first_bad;
    __shared__ u64 wsum[FRAME_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const u64 npos = *a.total < a.limit ? *a.total : a.limit;
    if (tid == 0) {
        u8 mode = 0;
        u64 count = 0, end = 0;
        const bool ok = read_header(a.t, a.n, &mode, &count, &end);
        hdr_ok = ok ? 1u : 0u;
        mode_sh = mode;
        count_sh = ok ? count : 0;
        nidx_sh = ok ? (count < (u64)a.max_blocks ? count : (u64)a.max_blocks) : 0;
        // the '@' before the count's digits: t[0], t[2] and t[1] when the mode character is one
        k0_sh = mode == '@' ? 3 : 2;
        // block 0 starts right behind the digits: the '@' of rank k0 must sit there
        first_bad = (ok && nidx_sh > 0 && !(k0_sh < npos && a.pos[k0_sh] == end)) ? 0 : 0x7FFFFFFF;
        maxsz_sh = 0;
        run_sh = 0;
        if (!ok) set_error(a.err, SHAFA_FILE_STREAM_FAILED);
    }
    __syncthreads();
    const u64 nidx = nidx_sh, k0 = k0_sh;
    for (int b0 = 0; b0 < a.max_blocks; b0 += FRAME_THREADS) {
        const int b = b0 + (int)tid;
        bool ok = false;
        u64 size = 0, ts = 0, tn = 0;
        if ((u64)b < nidx && b0 < first_bad) {
            const u64 j = k0 + 2 * (u64)b;                       // "@" <size> "@" <text> "@"
            if (j + 2 < npos) {
                const u64 p0 = a.pos[j], p1 = a.pos[j + 1], p2 = a.pos[j + 2];
                ok = p1 > p0 + 1 && p2 - p1 - 1 >= 1 && p2 - p1 - 1 <= a.field_max;
                for (u64 p = p0 + 1; ok && p < p1; ++p) {
                    const u8 c = a.t[p];
                    if (!is_digit(c)) ok = false;
                    size = size * 10 + (u64)(c - '0');
                }
                ts = p1 + 1;
                tn = p2 - p1 - 1;
            }
        }
        u64 incl = 0;
        if (a.off) {                                             // the .rle payloads: each must end inside the .rle
            const u64 v = ok ? (size < a.rle_n + 1 ? size : a.rle_n + 1) : 0;
            incl = wave_incl_scan_sat(v);
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            u64 before = run_sh;
            for (u32 w = 0; w < wv; ++w) before = sat_add(before, wsum[w]);
            incl = sat_add(before, incl);
            if (ok && incl > a.rle_n) ok = false;
        }
        if ((u64)b < nidx && b0 < first_bad && !ok) atomicMin(&first_bad, b);
        __syncthreads();
        const bool valid = (u64)b < nidx && b < first_bad;
        if (b < a.max_blocks) {
            a.sizes[b] = valid ? size : 0;
            if (a.spans) a.spans[b] = valid ? TextSpan{ts + span_base, tn} : TextSpan{0, 0};
            if (a.off) a.off[b] = valid ? incl - size + off_base : 0;
            if ((u64)b < nidx && b == first_bad) set_error(a.err + b, SHAFA_FILE_STREAM_FAILED);
            if (valid) atomicMax((unsigned long long *)&maxsz_sh, (unsigned long long)size);
        }
        if (a.off && wv == FRAME_THREADS / 64 - 1 && lane == 63) run_sh = incl;      // the last lane's sum, saturated
        __syncthreads();
    }
    if (tid == 0) {
        const u64 framed = (u64)first_bad < nidx ? (u64)first_bad : nidx;
        a.info[SHAFA_UNPACK_INFO_STATUS] = hdr_ok ? SHAFA_SUCCESS : SHAFA_FILE_STREAM_FAILED;
        a.info[SHAFA_UNPACK_INFO_MODE] = mode_sh;
        a.info[SHAFA_UNPACK_INFO_COUNT] = count_sh;
        a.info[SHAFA_UNPACK_INFO_INDEXED] = nidx;
        a.info[SHAFA_UNPACK_INFO_FRAMED] = framed;
        a.info[SHAFA_UNPACK_INFO_MAX_SIZE] = maxsz_sh;
    }
}

__global__ __launch_bounds__(FRAME_THREADS) void unpack_frames(FrameArgs a)
{
    frames(a, 0, 0);
}

// shafa_cod_parse (host/formats.c) on one block's text: only '0', '1' and ';' up to the text's first NUL byte, exactly 255
// ';', at most 255 characters a field.  Anything else: an all-empty table and SHAFA_FILE_UNRECOGNIZABLE.  A block that was not
// framed (span of 0 bytes) gets an all-empty table and no error.
__global__ __launch_bounds__(256) void unpack_tables(const u8 *__restrict__ t, const TextSpan *__restrict__ spans,
                                                     shafa_code_table *__restrict__ tabs, int *__restrict__ err)
{
    __shared__ u8 txt[COD_TEXT_MAX + 1];
    __shared__ u32 semi[256];
    __shared__ u32 wsum[4];
    __shared__ u32 nul, bad;
    const int b = blockIdx.x;
    const u32 s = threadIdx.x, lane = s & 63u, wv = s >> 6;
    const TextSpan sp = spans[b];
    const u32 n = (u32)sp.n;                                      // <= COD_TEXT_MAX (unpack_frames checked it)
    if (s == 0) {
        nul = n;
        bad = 0;
    }
    __syncthreads();
    for (u32 i = s; i < n; i += 256) {
        const u8 c = t[sp.start + i];
        txt[i] = c;
        if (c == 0) atomicMin(&nul, i);
    }
    __syncthreads();
    const u32 L = nul;                                            // the host parses a NUL-terminated string
    const u32 seg = (L + 255) / 256, lo = s * seg < L ? s * seg : L, hi = lo + seg < L ? lo + seg : L;
    u32 k = 0;
    bool odd = false;
    for (u32 i = lo; i < hi; ++i) {
        const u8 c = txt[i];
        if (c == ';') ++k;
        else if (c != '0' && c != '1') odd = true;
    }
    const u32 incl = dpp_scan_add(k);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    u32 r = incl - k;
    for (u32 w = 0; w < wv; ++w) r += wsum[w];
    const u32 total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (odd || (n && total != 255)) atomicOr(&bad, 1u);
    if (total == 255)
        for (u32 i = lo; i < hi; ++i)
            if (txt[i] == ';') semi[r++] = i;
    __syncthreads();
    u32 f0 = 0, flen = 0;
    if (n && !bad) {
        f0 = s == 0 ? 0 : semi[s - 1] + 1;
        const u32 f1 = s == 255 ? L : semi[s];
        flen = f1 - f0;
        if (flen > 255) atomicOr(&bad, 1u);
    }
    __syncthreads();
    if (bad) flen = 0;
    shafa_code_table *tb = tabs + b;
    tb->len[s] = (u8)flen;
    for (u32 q = 0; q < 32; ++q) {
        u32 byte = 0;
        for (u32 i = 0; i < 8; ++i) {
            const u32 bit = q * 8 + i;
            if (bit < flen && txt[f0 + bit] == '1') byte |= 0x80u >> i;
        }
        tb->bits[s][q] = (u8)byte;
    }
    if (s == 0 && bad) set_error(err + b, SHAFA_FILE_UNRECOGNIZABLE);
}

// inclusive max-scan over the 64 lanes of a wave: dpp_scan_add's steps with max (0 is the identity: a lane without a source
// gets `old` = 0)
__device__ __forceinline__ u32 dpp_scan_max(u32 v)
{
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1,3
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2,3
    return v;
}

// shafa_freq_parse (host/formats.c) on one block's text: up to the text's first NUL byte only digits and exactly 255 ';', and a
// first field that is not empty.  A field's value is v = v * 10 + d over its digits (any number of them, wrapping); an empty
// field repeats the nearest non-empty one before it.  Anything else: 256 zero counts and SHAFA_FILE_UNRECOGNIZABLE.  A block
// that was not framed (span of 0 bytes) gets 256 zero counts and no error.
// The text comes in as the aligned 16-byte words of memory that hold it (each holds a byte of it), so it sits in LDS `lead`
// bytes behind the first word's start.
__global__ __launch_bounds__(256) void unpack_counts(const u8 *__restrict__ t, const TextSpan *__restrict__ spans,
                                                     u64 *__restrict__ counts, int *__restrict__ err)
{
    __shared__ uint4 words[FREQ_TEXT_WORDS];
    __shared__ u64 val[256];
    __shared__ u32 semi[256];
    __shared__ u32 wsum[4], wlast[4];
    __shared__ u32 nul, bad;
    const int b = blockIdx.x;
    const u32 s = threadIdx.x, lane = s & 63u, wv = s >> 6;
    const TextSpan sp = spans[b];
    const u32 n = (u32)sp.n;                                      // <= FREQ_TEXT_MAX (unpack_frames checked it)
    const u32 lead = n ? (u32)((uintptr_t)(t + sp.start) & 15) : 0;
    const u32 nw = (lead + n + 15) / 16;                          // <= FREQ_TEXT_WORDS
    if (s == 0) {
        nul = n;
        bad = 0;
    }
    for (u32 i = s; i < nw; i += 256) words[i] = gload<uint4>(t + sp.start - lead + (u64)i * 16);
    __syncthreads();
    const u8 *txt = (const u8 *)words + lead;
    // a lane per stretch of the text: its ';', its bytes that are neither ';' nor digit, up to its first NUL
    const u32 seg = (n + 255) / 256, lo = s * seg < n ? s * seg : n, hi = lo + seg < n ? lo + seg : n;
    u32 k = 0;
    bool odd = false;
    for (u32 i = lo; i < hi; ++i) {
        const u8 c = txt[i];
        if (c == 0) {
            atomicMin(&nul, i);
            break;
        }
        if (c == ';') ++k;
        else if (!is_digit(c)) odd = true;
    }
    __syncthreads();
    const u32 L = nul;                                            // the host parses a NUL-terminated string
    if (lo >= L) {                                                // behind the first NUL: not looked at
        k = 0;
        odd = false;
    }
    const u32 incl = dpp_scan_add(k);
    if (lane == 63) wsum[wv] = incl;
    if (odd || (s == 0 && n && (L == 0 || txt[0] == ';'))) atomicOr(&bad, 1u);      // field 0 must not be empty
    __syncthreads();
    u32 r = incl - k;
    for (u32 w = 0; w < wv; ++w) r += wsum[w];
    const u32 total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (s == 0 && n && total != 255) atomicOr(&bad, 1u);
    if (total == 255)
        for (u32 i = lo; i < hi && i < L; ++i)
            if (txt[i] == ';') semi[r++] = i;
    __syncthreads();
    const bool ok = n && !bad;
    u64 v = 0;
    u32 last = 0;                                                 // the last non-empty field up to this one (field 0 is one)
    if (ok) {
        const u32 f0 = s == 0 ? 0 : semi[s - 1] + 1, f1 = s == 255 ? L : semi[s];
        for (u32 i = f0; i < f1; ++i) v = v * 10 + (u64)(txt[i] - '0');
        if (f1 > f0) last = s;
    }
    val[s] = v;
    last = dpp_scan_max(last);
    if (lane == 63) wlast[wv] = last;
    __syncthreads();
    for (u32 w = 0; w < wv; ++w) last = max(last, wlast[w]);
    counts[(u64)b * 256 + s] = ok ? val[last] : 0;
    if (s == 0 && bad) set_error(err + b, SHAFA_FILE_UNRECOGNIZABLE);
}

// shaf_read_u64 (host/modules.c) at p: `lead`, 1..20 digits (a 21st is left unread), then '@' when trailing_at; the window is
// the 32 bytes the host's pread asks for, cut by the end of the file.  All 64 lanes call it.
__device__ bool shaf_read(const u8 *f, u64 n, u64 p, bool trailing_at, u64 *v, u64 *end)
{
    const u32 lane = (u32)lane_id();
    const u64 got = n - p < 32 ? n - p : 32;                     // p <= n
    const u8 c = lane < got ? f[p + lane] : 0;
    const u64 dig = __ballot(lane >= 1 && lane < got && is_digit(c));
    const u8 c0 = (u8)__shfl((int)c, 0, 64);
    const u32 digits_run = (u32)__builtin_ctzll(~(dig >> 1));     // consecutive digits from byte 1
    const u32 digits = digits_run < 20 ? digits_run : 20;
    if (got < 2 || c0 != '@' || digits == 0) return false;
    u64 i = 1 + digits;
    if (trailing_at) {
        const u8 ci = (u8)__shfl((int)c, (int)(i < 63 ? i : 63), 64);
        if (i >= got || ci != '@') return false;
        ++i;
    }
    // x = x * 10 + d over the digits, wrapping: the sum of d_k * 10^(digits - k) mod 2^64
    u64 term = 0;
    if (lane >= 1 && lane <= digits) {
        u64 pw = 1;
        for (u32 e = lane; e < digits; ++e) pw *= 10;
        term = (u64)(c - '0') * pw;
    }
    for (int d = 32; d >= 1; d >>= 1) term += __shfl_xor(term, d, 64);
    *v = term;
    *end = p + i;
    return true;
}

// "@<n>", then per block "@<size>@" + size payload bytes, for min(want, max_blocks) blocks: a dependent chain, one wave.
// Payload offsets are written off_base bytes further on (the segmented form: from the call's base pointer).
__device__ __forceinline__ void shaf_walk(const u8 *__restrict__ f, u64 n, u64 want, int max_blocks, u64 *__restrict__ off,
                                          u64 *__restrict__ sz, int *__restrict__ err, u64 off_base)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 nb = want < (u64)max_blocks ? want : (u64)max_blocks;
    u64 v = 0, p = 0;
    bool ok = shaf_read(f, n, 0, false, &v, &p);                  // d.c:673: read, then overruled by the .cod's count
    u64 b = 0;
    // the host reads block b's .shaf header and payload before its .cod text: a failure here replaces the table error that
    // unpack_tables may have left on the same block
    if (!ok && lane == 0) set_error_over(err, SHAFA_FILE_STREAM_FAILED, SHAFA_FILE_UNRECOGNIZABLE);
    for (; ok && b < nb; ++b) {
        u64 end = 0;
        ok = shaf_read(f, n, p, true, &v, &end) && v <= n - end;  // the payload ends inside the file
        if (!ok) {
            if (lane == 0) set_error_over(err + b, SHAFA_FILE_STREAM_FAILED, SHAFA_FILE_UNRECOGNIZABLE);
            break;
        }
        if (lane == 0) {
            off[b] = end + off_base;
            sz[b] = v;
        }
        p = end + v;
    }
    for (u64 i = b + lane; i < (u64)max_blocks; i += 64) {
        off[i] = 0;
        sz[i] = 0;
    }
}

__global__ __launch_bounds__(64) void unpack_shaf_walk(const u8 *__restrict__ f, u64 n, const u64 *__restrict__ count,
                                                      int max_blocks, u64 *__restrict__ off, u64 *__restrict__ sz,
                                                      int *__restrict__ err)
{
    shaf_walk(f, n, *count, max_blocks, off, sz, err, 0);
}

// ---- segmented parse: many files in one launch sequence --------------------------------------------------------------
// File f's bytes are [t, t + n) (the call's base + its offset); its blocks take slots first .. first + max_blocks - 1 of the
// call's arrays and of the batch's error words.  A text's 4 KiB chunks are entries pair0 .. pair0 + nchunks - 1 of the call's
// (file, chunk) list, its '@' positions entries pos0 .. pos0 + limit - 1 of the workspace.
struct TextFile {
    const u8 *t;
    u64 n;
    u64 span_base;           // t - the call's text base: unpack_tables reads the spans as offsets from that base
    u64 rle_n;               // .freq: its .rle's length
    u64 off_base;            // .freq: its .rle's offset from the call's .rle base
    u64 pos0, limit;
    u32 pair0, nchunks;
    int first, max_blocks;
};

struct ShafFile {
    const u8 *f;
    u64 n;
    u64 off_base;            // f - the call's base
    int first, max_blocks;
};

// a workgroup per (file, chunk) pair: the chunk's '@' count
__global__ __launch_bounds__(IDX_THREADS) void unpack_at_count_files(const TextFile *__restrict__ files,
                                                                     const u32 *__restrict__ pair_file, u32 *__restrict__ cnt)
{
    const u32 p = blockIdx.x;
    const TextFile &tf = files[pair_file[p]];
    at_count(tf.t, tf.n, p - tf.pair0, cnt + p);
}

// a workgroup per pair.  base: the exclusive scan of every pair's count (unpack_at_scan over the whole list, base[npairs] =
// the sum), so a file's ranks are differences from its first chunk's base.  The file's first chunk also writes its total.
__global__ __launch_bounds__(IDX_THREADS) void unpack_at_place_files(const TextFile *__restrict__ files,
                                                                     const u32 *__restrict__ pair_file,
                                                                     const u64 *__restrict__ base, u64 *__restrict__ total,
                                                                     u64 *__restrict__ pos)
{
    const u32 p = blockIdx.x, f = pair_file[p];
    const TextFile &tf = files[f];
    const u64 b_file = base[tf.pair0];
    if (p == tf.pair0 && threadIdx.x == 0) total[f] = base[tf.pair0 + tf.nchunks] - b_file;
    at_place(tf.t, tf.n, p - tf.pair0, base[p] - b_file, tf.limit, pos + tf.pos0);
}

struct FramesFilesArgs {
    const TextFile *files;
    const u64 *total;        // per file: its '@' count
    const u64 *pos;
    u32 field_max;
    u64 *info;               // SHAFA_UNPACK_INFO_WORDS per file
    u64 *sizes;              // per slot
    TextSpan *spans;         // per slot: .cod; nullptr for .freq
    u64 *off;                // per slot: .freq; nullptr for .cod
    int *err;                // per slot
};

// a workgroup per file: unpack_frames on its text
__global__ __launch_bounds__(FRAME_THREADS) void unpack_frames_files(FramesFilesArgs g)
{
    const u32 f = blockIdx.x;
    const TextFile tf = g.files[f];
    FrameArgs a = {};
    a.t = tf.t;
    a.n = tf.n;
    a.total = g.total + f;
    a.pos = g.pos + tf.pos0;
    a.limit = tf.limit;
    a.max_blocks = tf.max_blocks;
    a.field_max = g.field_max;
    a.info = g.info + (u64)f * SHAFA_UNPACK_INFO_WORDS;
    a.sizes = g.sizes + tf.first;
    a.spans = g.spans ? g.spans + tf.first : nullptr;
    a.off = g.off ? g.off + tf.first : nullptr;
    a.rle_n = tf.rle_n;
    a.err = g.err + tf.first;
    frames(a, tf.span_base, tf.off_base);
}

// a wave per file: unpack_shaf_walk on its .shaf, its block count at count[f * SHAFA_UNPACK_INFO_WORDS]
__global__ __launch_bounds__(64) void unpack_shaf_walk_files(const ShafFile *__restrict__ files, const u64 *__restrict__ count,
                                                            u64 *__restrict__ off, u64 *__restrict__ sz, int *__restrict__ err)
{
    const ShafFile sf = files[blockIdx.x];
    shaf_walk(sf.f, sf.n, count[(u64)blockIdx.x * SHAFA_UNPACK_INFO_WORDS], sf.max_blocks, off + sf.first, sz + sf.first,
              err + sf.first, sf.off_base);
}

struct MoveRegion {
    u8 *dst;
    u64 cap;
};

// block b: [file + d_off[b], + d_n[b]) -> regions[b].dst.  Two records per block for pack.hip's movers: pack_seams takes the
// payload as it is; pack_bulk's source must be 16-aligned, so its record starts (src & 15) bytes early on both sides — the
// same whole destination words (the destination is aligned), each loaded from the word that holds its first payload byte.
__global__ __launch_bounds__(64) void unpack_move_plan(int nblocks, const u8 *file, u64 file_n, const u64 *__restrict__ d_off,
                                                       const u64 *__restrict__ d_n, const MoveRegion *__restrict__ regions,
                                                       MoveDesc *__restrict__ bulk, MoveDesc *__restrict__ seam,
                                                       u32 *__restrict__ verdict, int *__restrict__ err)
{
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b == 0) *verdict = 1;
    if (b >= nblocks) return;
    const MoveRegion r = regions[b];
    u64 n = d_n[b];
    const u64 o = d_off[b];
    if (n > r.cap || o > file_n || n > file_n - o) {
        set_error(err + b, SHAFA_OUTSIDE_MODULE);
        n = 0;
    }
    const u8 *src = file + (n ? o : 0);
    const u64 delta = n ? (u64)(uintptr_t)src & 15 : 0;
    MoveDesc d = {};
    d.src = src;
    d.dst = r.dst;
    d.n = n;
    seam[b] = d;
    d.src = src - delta;
    d.dst = r.dst - delta;
    d.n = n + delta;
    bulk[b] = d;
}

size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

int idx_ws(Batch *bt, hipStream_t st, u64 n, int max_blocks, bool spans, u64 limit, IdxWs &w)
{
    const u64 nchunks = n ? ceil_div_u64(n, IDX_CHUNK) : 1;
    const size_t o_cnt = 16, o_base = o_cnt + al16(nchunks * 4), o_pos = o_base + al16(nchunks * 8),
                 o_spans = o_pos + al16(limit * 8), bytes = o_spans + (spans ? (size_t)max_blocks * sizeof(TextSpan) : 0);
    if (int rc = batch_reserve(bt, st, bytes)) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    w.total = (u64 *)ws;
    w.cnt = (u32 *)(ws + o_cnt);
    w.base = (u64 *)(ws + o_base);
    w.pos = (u64 *)(ws + o_pos);
    w.spans = spans ? (TextSpan *)(ws + o_spans) : nullptr;
    return SHAFA_SUCCESS;
}

// the '@' index of a text, then its frames (and, for a .cod, its tables; for a .freq's fields, its counts)
int text_unpack(Batch *bt, hipStream_t st, int max_blocks, const u8 *d_text, u64 n, u32 field_max, u64 *d_info, u64 *d_sizes,
                shafa_code_table *d_tables, u64 *d_off, u64 rle_n, u64 *d_counts = nullptr)
{
    IdxWs w;
    const u64 limit = 2 * (u64)max_blocks + 4;                    // the header's 2 or 3, then two per block, and the last one
    if (int rc = idx_ws(bt, st, n, max_blocks, d_tables || d_counts, limit, w)) return rc;
    const u64 nchunks = n ? ceil_div_u64(n, IDX_CHUNK) : 1;
    if (nchunks > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    hipLaunchKernelGGL(unpack_at_count, dim3((u32)nchunks), dim3(IDX_THREADS), 0, st, d_text, n, w.cnt);
    hipLaunchKernelGGL(unpack_at_scan, dim3(1), dim3(IDX_THREADS), 0, st, (const u32 *)w.cnt, nchunks, w.base, w.total);
    hipLaunchKernelGGL(unpack_at_place, dim3((u32)nchunks), dim3(IDX_THREADS), 0, st, d_text, n, (const u64 *)w.base, limit,
                       w.pos);
    FrameArgs a = {};
    a.t = d_text;
    a.n = n;
    a.total = w.total;
    a.pos = w.pos;
    a.limit = limit;
    a.max_blocks = max_blocks;
    a.field_max = field_max;
    a.info = d_info;
    a.sizes = d_sizes;
    a.spans = w.spans;
    a.off = d_off;
    a.rle_n = rle_n;
    a.err = bt->d_err;
    hipLaunchKernelGGL(unpack_frames, dim3(1), dim3(FRAME_THREADS), 0, st, a);
    if (d_tables)
        hipLaunchKernelGGL(unpack_tables, dim3((u32)max_blocks), dim3(256), 0, st, d_text, (const TextSpan *)w.spans, d_tables,
                           bt->d_err);
    if (d_counts)
        hipLaunchKernelGGL(unpack_counts, dim3((u32)max_blocks), dim3(256), 0, st, d_text, (const TextSpan *)w.spans, d_counts,
                           bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

int move_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_file, u64 file_n, const u64 *d_off, const u64 *d_n,
                u8 *d_dst, const u64 *h_dst_off, const u64 *h_dst_cap)
{
    const size_t o_bulk = 256, o_seam = o_bulk + al16((size_t)nblocks * sizeof(MoveDesc));
    if (int rc = batch_reserve(bt, st, o_seam + (size_t)nblocks * sizeof(MoveDesc))) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    u32 *verdict = (u32 *)ws;
    MoveDesc *bulk = (MoveDesc *)(ws + o_bulk), *seam = (MoveDesc *)(ws + o_seam);
    u64 max_cap = 0;
    for (int b = 0; b < nblocks; ++b)
        if (h_dst_cap[b] > max_cap) max_cap = h_dst_cap[b];
    const size_t par_bytes = (size_t)nblocks * sizeof(MoveRegion);
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    MoveRegion *hp = (MoveRegion *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    for (int b = 0; b < nblocks; ++b) {
        hp[b].dst = d_dst + h_dst_off[b];
        hp[b].cap = h_dst_cap[b];
    }
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    hipLaunchKernelGGL(unpack_move_plan, dim3((u32)ceil_div_u64((u64)nblocks, 64)), dim3(64), 0, st, nblocks, d_file, file_n,
                       d_off, d_n, (const MoveRegion *)dpar, bulk, seam, verdict, bt->d_err);
    if (int rc = pack_move_launch(st, nblocks, bulk, seam, verdict, max_cap)) return rc;
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

// the files' slot ranges, (first, max_blocks) sorted by first
std::vector<std::pair<int, int>> slot_ranges(int nfiles, const int *h_first, const int *h_max_blocks)
{
    std::vector<std::pair<int, int>> r((size_t)nfiles);
    for (int f = 0; f < nfiles; ++f) r[(size_t)f] = {h_first[f], h_max_blocks[f]};
    std::sort(r.begin(), r.end());
    return r;
}

// argument checks shared by the three segmented entries (no HIP call)
int files_check(const Batch *bt, int nfiles, const int *h_first, const int *h_max_blocks, const void *base, const u64 *h_off,
                const u64 *h_n)
{
    if (!bt || nfiles < 1 || !h_first || !h_max_blocks || !h_off || !h_n) return SHAFA_OUTSIDE_MODULE;
    long long slots = 0;
    for (int f = 0; f < nfiles; ++f) {
        const long long first = h_first[f], mb = h_max_blocks[f];
        if (mb < 1 || first < 0 || first + mb > bt->max_blocks) return SHAFA_OUTSIDE_MODULE;
        if (!base && h_n[f]) return SHAFA_OUTSIDE_MODULE;
        slots += mb;
    }
    const std::vector<std::pair<int, int>> r = slot_ranges(nfiles, h_first, h_max_blocks);
    for (size_t i = 1; i < r.size(); ++i)
        if ((long long)r[i - 1].first + r[i - 1].second > r[i].first) return SHAFA_OUTSIDE_MODULE;
    if (slots > 0x7FFFFFFFll) return SHAFA_LACK_OF_MEMORY;
    return SHAFA_SUCCESS;
}

// the '@' index of every text, then their frames (and, for .cod, their tables): text_unpack per file, one launch sequence
int text_files_unpack(Batch *bt, hipStream_t st, int nfiles, const int *h_first, const int *h_max_blocks, const u8 *d_text,
                      const u64 *h_text_off, const u64 *h_text_n, u32 field_max, u64 *d_info, u64 *d_sizes,
                      shafa_code_table *d_tables, u64 *d_off, const u64 *h_rle_off, const u64 *h_rle_n)
{
    u64 npairs = 0, npos = 0;
    int slot_end = 0;
    for (int f = 0; f < nfiles; ++f) {
        npairs += h_text_n[f] ? ceil_div_u64(h_text_n[f], IDX_CHUNK) : 1;
        npos += 2 * (u64)h_max_blocks[f] + 4;
        if (h_first[f] + h_max_blocks[f] > slot_end) slot_end = h_first[f] + h_max_blocks[f];
    }
    if (npairs > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    // workspace: [pair bases: npairs + 1][file totals][pair counts][positions][spans per slot, .cod only]
    const size_t o_total = al16((npairs + 1) * 8), o_cnt = o_total + al16((size_t)nfiles * 8),
                 o_pos = o_cnt + al16(npairs * 4), o_spans = o_pos + al16(npos * 8),
                 bytes = o_spans + (d_tables ? (size_t)slot_end * sizeof(TextSpan) : 0);
    if (int rc = batch_reserve(bt, st, bytes)) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    u64 *base = (u64 *)ws, *total = (u64 *)(ws + o_total), *pos = (u64 *)(ws + o_pos);
    u32 *cnt = (u32 *)(ws + o_cnt);
    TextSpan *spans = d_tables ? (TextSpan *)(ws + o_spans) : nullptr;
    const size_t o_pairs = (size_t)nfiles * sizeof(TextFile), par_bytes = o_pairs + npairs * 4;
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    TextFile *hp = (TextFile *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    u32 *hpair = (u32 *)((u8 *)hp + o_pairs);
    u64 pair = 0, p0 = 0;
    for (int f = 0; f < nfiles; ++f) {
        const u64 n = h_text_n[f], nch = n ? ceil_div_u64(n, IDX_CHUNK) : 1;
        TextFile &t = hp[f];
        t.t = d_text + (n ? h_text_off[f] : 0);
        t.n = n;
        t.span_base = n ? h_text_off[f] : 0;
        t.rle_n = h_rle_n ? h_rle_n[f] : 0;
        t.off_base = h_rle_off ? h_rle_off[f] : 0;
        t.pos0 = p0;
        t.limit = 2 * (u64)h_max_blocks[f] + 4;         // the header's 2 or 3, then two per block, and the last one
        t.pair0 = (u32)pair;
        t.nchunks = (u32)nch;
        t.first = h_first[f];
        t.max_blocks = h_max_blocks[f];
        for (u64 c = 0; c < nch; ++c) hpair[pair++] = (u32)f;
        p0 += t.limit;
    }
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    const TextFile *d_files = (const TextFile *)dpar;
    const u32 *d_pair = (const u32 *)(dpar + o_pairs);
    hipLaunchKernelGGL(unpack_at_count_files, dim3((u32)npairs), dim3(IDX_THREADS), 0, st, d_files, d_pair, cnt);
    hipLaunchKernelGGL(unpack_at_scan, dim3(1), dim3(IDX_THREADS), 0, st, (const u32 *)cnt, npairs, base, base + npairs);
    hipLaunchKernelGGL(unpack_at_place_files, dim3((u32)npairs), dim3(IDX_THREADS), 0, st, d_files, d_pair, (const u64 *)base,
                       total, pos);
    FramesFilesArgs g = {};
    g.files = d_files;
    g.total = total;
    g.pos = pos;
    g.field_max = field_max;
    g.info = d_info;
    g.sizes = d_sizes;
    g.spans = spans;
    g.off = d_off;
    g.err = bt->d_err;
    hipLaunchKernelGGL(unpack_frames_files, dim3((u32)nfiles), dim3(FRAME_THREADS), 0, st, g);
    if (d_tables) {                                   // one launch per run of consecutive slots: none between files is written
        const std::vector<std::pair<int, int>> r = slot_ranges(nfiles, h_first, h_max_blocks);
        for (size_t i = 0; i < r.size();) {
            const int s0 = r[i].first;
            int s1 = s0 + r[i].second;
            for (++i; i < r.size() && r[i].first == s1; ++i) s1 += r[i].second;
            hipLaunchKernelGGL(unpack_tables, dim3((u32)(s1 - s0)), dim3(256), 0, st, d_text, (const TextSpan *)(spans + s0),
                               d_tables + s0, bt->d_err + s0);
        }
    }
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

int shaf_files_unpack(Batch *bt, hipStream_t st, int nfiles, const int *h_first, const int *h_max_blocks, const u8 *d_shaf,
                      const u64 *h_shaf_off, const u64 *h_shaf_n, const u64 *d_count, u64 *d_off, u64 *d_n)
{
    const size_t par_bytes = (size_t)nfiles * sizeof(ShafFile);
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    ShafFile *hp = (ShafFile *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    for (int f = 0; f < nfiles; ++f) {
        const u64 n = h_shaf_n[f], o = n ? h_shaf_off[f] : 0;
        hp[f].f = d_shaf + o;
        hp[f].n = n;
        hp[f].off_base = o;
        hp[f].first = h_first[f];
        hp[f].max_blocks = h_max_blocks[f];
    }
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    hipLaunchKernelGGL(unpack_shaf_walk_files, dim3((u32)nfiles), dim3(64), 0, st, (const ShafFile *)dpar, d_count, d_off, d_n,
                       bt->d_err);
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

}  // namespace

extern "C" {

int shafa_hipd_unpack_cod(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_cod, uint64_t cod_n,
                          uint64_t *d_info, uint64_t *d_sizes, shafa_code_table *d_tables)
{
    if (!b || max_blocks < 1 || (!d_cod && cod_n) || !d_info || !d_sizes || !d_tables) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (max_blocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_unpack(bt, (hipStream_t)stream, max_blocks, d_cod, cod_n, COD_TEXT_MAX, d_info, d_sizes, d_tables, nullptr, 0);
}

int shafa_hipd_unpack_rle_freq(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_freq, uint64_t freq_n,
                               uint64_t rle_n, uint64_t *d_info, uint64_t *d_off, uint64_t *d_n)
{
    if (!b || max_blocks < 1 || (!d_freq && freq_n) || !d_info || !d_off || !d_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (max_blocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_unpack(bt, (hipStream_t)stream, max_blocks, d_freq, freq_n, FREQ_TEXT_MAX, d_info, d_n, nullptr, d_off, rle_n);
}

int shafa_hipd_unpack_freq(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_freq_text, uint64_t freq_n,
                           uint64_t *d_info, uint64_t *d_sizes, uint64_t *d_counts)
{
    if (!b || max_blocks < 1 || (!d_freq_text && freq_n) || !d_info || !d_sizes || !d_counts) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (max_blocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_unpack(bt, (hipStream_t)stream, max_blocks, d_freq_text, freq_n, FREQ_TEXT_MAX, d_info, d_sizes, nullptr,
                       nullptr, 0, d_counts);
}

int shafa_hipd_unpack_shaf(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_shaf, uint64_t shaf_n,
                           const uint64_t *d_count, uint64_t *d_off, uint64_t *d_n)
{
    if (!b || max_blocks < 1 || (!d_shaf && shaf_n) || !d_count || !d_off || !d_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (max_blocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = batch_enter(bt, st)) return rc;
    hipLaunchKernelGGL(unpack_shaf_walk, dim3(1), dim3(64), 0, st, d_shaf, shaf_n, d_count, max_blocks, d_off, d_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

int shafa_hipd_unpack_payloads(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_file, uint64_t file_n,
                               const uint64_t *d_off, const uint64_t *d_n, uint8_t *d_dst, const uint64_t *h_dst_off,
                               const uint64_t *h_dst_cap)
{
    if (!b || nblocks < 1 || (!d_file && file_n) || !d_off || !d_n || !d_dst || !h_dst_off || !h_dst_cap)
        return SHAFA_OUTSIDE_MODULE;
    if ((uintptr_t)d_dst & 15) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (h_dst_off[i] & 15) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (nblocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return move_launch(bt, (hipStream_t)stream, nblocks, d_file, file_n, d_off, d_n, d_dst, h_dst_off, h_dst_cap);
}

int shafa_hipd_unpack_cod_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_max_blocks,
                                const uint8_t *d_text, const uint64_t *h_text_off, const uint64_t *h_text_n,
                                uint64_t *d_info, uint64_t *d_sizes, shafa_code_table *d_tables)
{
    if (!d_info || !d_sizes || !d_tables) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (int rc = files_check(bt, nfiles, h_first, h_max_blocks, d_text, h_text_off, h_text_n)) return rc;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_files_unpack(bt, (hipStream_t)stream, nfiles, h_first, h_max_blocks, d_text, h_text_off, h_text_n, COD_TEXT_MAX,
                             d_info, d_sizes, d_tables, nullptr, nullptr, nullptr);
}

int shafa_hipd_unpack_rle_freq_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first,
                                     const int *h_max_blocks, const uint8_t *d_text, const uint64_t *h_text_off,
                                     const uint64_t *h_text_n, const uint64_t *h_rle_off, const uint64_t *h_rle_n,
                                     uint64_t *d_info, uint64_t *d_off, uint64_t *d_n)
{
    if (!h_rle_off || !h_rle_n || !d_info || !d_off || !d_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (int rc = files_check(bt, nfiles, h_first, h_max_blocks, d_text, h_text_off, h_text_n)) return rc;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_files_unpack(bt, (hipStream_t)stream, nfiles, h_first, h_max_blocks, d_text, h_text_off, h_text_n,
                             FREQ_TEXT_MAX, d_info, d_n, nullptr, d_off, h_rle_off, h_rle_n);
}

int shafa_hipd_unpack_shaf_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_max_blocks,
                                 const uint8_t *d_shaf, const uint64_t *h_shaf_off, const uint64_t *h_shaf_n,
                                 const uint64_t *d_count, uint64_t *d_off, uint64_t *d_n)
{
    if (!d_count || !d_off || !d_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    if (int rc = files_check(bt, nfiles, h_first, h_max_blocks, d_shaf, h_shaf_off, h_shaf_n)) return rc;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return shaf_files_unpack(bt, (hipStream_t)stream, nfiles, h_first, h_max_blocks, d_shaf, h_shaf_off, h_shaf_n, d_count,
                             d_off, d_n);
}

}  // extern "C"
