// pack.hip — the project's four file formats assembled in device memory (shafa_hipd_pack_payloads / _pack_cod / _pack_freq).
//
// What the device entries leave — payloads at the start of worst-case regions, sizes in device arrays, codes in binary tables,
// counts in 256-bin histograms — becomes ONE contiguous file, byte for byte what the C host writes (host/modules.c, with
// host/formats.c's shafa_cod_format / shafa_freq_format):
//   .rle   payloads back to back                                              (f.c:307)
//   .shaf  "@<n>", then "@<size>@" + payload per block                         (c.c:351,256-258)
//   .cod   "@<mode>@<n>", then "@<size>@" + "c0;c1;...;c255" per block, "@0"   (t.c:302,353-361,395-396)
//   .freq  "@<mode>@<n>", then "@<size>@" + make_freq's text per block, "@0"  (f.c:89-119)
//
// Kernels (stable names for rocprofv3):
//   pack_measure<CodText | FreqText>       one workgroup per block, a lane per symbol: the block's text length
//   pack_plan                              ONE workgroup looping over the blocks: header lengths, the exclusive scan of the
//                                          frames, the capacity checks, *d_dst_n, a descriptor per block and the verdict
//   pack_bulk                              the payloads' aligned 16-byte destination words (the hot path)
//   pack_seams                             a lane per block: "@n", "@size@" and the partial words at both ends of a payload
//   pack_text<CodText | FreqText>          one workgroup per block, a lane per symbol: header and fields
// Every later kernel reads the verdict word first and returns when the plan refused the file: then no byte of d_dst is written.
// Segmented packs (shafa_hipd_pack_*_files: many files in one launch sequence) add
//   pack_file_plan                         one workgroup per file: pack_plan's scan and checks (plan_frames) over the file's
//                                          blocks, its length and its verdict; a refused file's descriptors get n = 0, hdr_len = 0
//   pack_file_text<CodText | FreqText>     pack_text without the file's head and tail (text_frame), per descriptor slot
//   pack_file_ends                         a lane per file: its "@<n>" / "@<mode>@<n>" head and its "@0" tail
// and run pack_measure, pack_bulk and pack_seams as they are.
//
// Byte ownership (payloads).  With P = a payload's first destination byte and n its size, the words [ceil(P/16), floor((P+n)/16))
// lie entirely inside the payload: pack_bulk writes them, whole, with aligned 16-byte stores (an unaligned store is serialised
// lane by lane on gfx950).  Every other byte of the file — the headers and the 0..15 bytes at each end of a
// payload — is pack_seams', written one byte at a time.  The two kernels share 16-byte words but never a byte.
#include "common.hpp"
#include "internal.hpp"

namespace {

constexpr int PLAN_THREADS = 256;
constexpr int BULK_THREADS = 256;
constexpr int BULK_WORDS = 8;                                // 16-byte words per lane and pass, loads issued before stores
constexpr int BULK_PASSES = 2;
constexpr u64 BULK_CHUNK_WORDS = (u64)BULK_THREADS * BULK_WORDS * BULK_PASSES;   // 64 KiB of destination per workgroup

// one block's frame: [dst, dst + hdr_len) = "@<hdr_val>@" (hdr_len 0: none), then n body bytes (copied from src for payloads)
struct PackDesc {
    const u8 *src;
    u8 *dst;
    u64 n;
    u64 hdr_val;
    u32 hdr_len;
    u32 pad;
};

// host-known per block (payloads only), uploaded with the launch
struct PackSrc {
    const u8 *src;
    u64 cap;
};

// what a plan reads per block of the call, for one file (pack_plan) or many (pack_file_plan)
struct PlanBlocks {
    u32 hdr;                 // 1: every block's frame starts with "@<size>@"
    const PackSrc *srcs;     // payloads: sources and capacities; text: nullptr
    const u64 *n;            // body sizes: d_src_n (payloads) or the measure kernel's lengths (text)
    const u64 *hdr_vals;     // the numbers of the block headers: nullptr = the body sizes
    PackDesc *desc;
    u32 *verdict;            // the movers' word.  One file: 1 to write it, 0: refused (bad size, or too long for dst_cap)
    int *err;                // per block
};

struct PlanArgs {
    PlanBlocks blk;
    int nblocks;
    u64 head_len, tail_len;  // the file's prefix and suffix ("@<n>", "@<mode>@<n>", "@0")
    u8 *dst;
    u64 dst_cap;
    u64 *dst_n;
};

__host__ __device__ inline u32 dec_digits(u64 v)
{
    u32 d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// v in decimal at p, exactly dec_digits(v) bytes
__device__ inline u8 *put_dec(u8 *p, u64 v)
{
    const u32 d = dec_digits(v);
    for (u32 i = d; i-- > 0;) { p[i] = (u8)('0' + (u32)(v % 10)); v /= 10; }
    return p + d;
}

// workgroup-wide exclusive sum of u64 (PLAN_THREADS lanes); *total = the sum over all lanes
__device__ inline u64 wg_excl_scan(u64 v, u64 *wsum, u64 *total)
{
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const u64 incl = wave_incl_scan_add<u64>(v);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    u64 base = 0, all = 0;
    for (u32 w = 0; w < PLAN_THREADS / 64; ++w) {
        if (w < wv) base += wsum[w];
        all += wsum[w];
    }
    __syncthreads();                                 // wsum is reused by the next call
    *total = all;
    return base + incl - v;
}

// One workgroup plans one file: blocks first .. first + count - 1 of the call's arrays, their descriptors at desc[0 .. count),
// their frames back to back from dst + head_len.  Header lengths, the exclusive scan of the frames, the capacity checks, *dst_n
// and the verdict, which thread 0 returns (1: write the file); a file too long for cap is reported in *err_long.
__device__ __forceinline__ u32 plan_frames(const PlanBlocks &a, int first, int count, PackDesc *desc, u8 *dst, u64 cap,
                                           u64 head_len, u64 tail_len, u64 *dst_n, int *err_long)
{
    __shared__ u64 wsum[PLAN_THREADS / 64];
    __shared__ u32 bad_sh;
    const u32 tid = threadIdx.x;
    if (tid == 0) bad_sh = 0;
    __syncthreads();
    u64 pos = head_len;                              // the next frame's offset in the file
    for (int i0 = 0; i0 < count; i0 += PLAN_THREADS) {
        const int i = i0 + (int)tid;
        u64 frame = 0;
        PackDesc d = {};
        if (i < count) {
            const int b = first + i;
            const u64 n = a.n[b];
            if (a.srcs) {
                const PackSrc s = a.srcs[b];
                if (n > s.cap) {
                    set_error(a.err + b, SHAFA_OUTSIDE_MODULE);
                    atomicOr(&bad_sh, 1u);
                }
                d.src = s.src;
            }
            d.n = n;
            d.hdr_val = a.hdr_vals ? a.hdr_vals[b] : n;
            d.hdr_len = a.hdr ? 2u + dec_digits(d.hdr_val) : 0u;
            frame = d.hdr_len + n;
        }
        u64 sum;
        const u64 off = pos + wg_excl_scan(frame, wsum, &sum);
        if (i < count) {
            d.dst = dst + off;
            desc[i] = d;
        }
        pos += sum;
    }
    __syncthreads();
    u32 go = 1;
    if (tid == 0) {
        const u64 total = pos + tail_len;
        if (bad_sh) {
            go = 0;
            *dst_n = 0;
        } else {
            *dst_n = total;
            if (total > cap) {
                set_error(err_long, SHAFA_LACK_OF_MEMORY);
                go = 0;
            }
        }
    }
    return go;
}

__global__ __launch_bounds__(PLAN_THREADS) void pack_plan(PlanArgs a)
{
    const u32 go = plan_frames(a.blk, 0, a.nblocks, a.blk.desc, a.dst, a.dst_cap, a.head_len, a.tail_len, a.dst_n, a.blk.err);
    if (threadIdx.x == 0) *a.blk.verdict = go;
}

// the destination words of a payload that lie entirely inside it: [w_lo, w_hi) in units of 16 bytes of address
__device__ inline void whole_words(const PackDesc &d, u64 &w_lo, u64 &w_hi)
{
    const u64 p = (u64)(uintptr_t)(d.dst + d.hdr_len);
    w_lo = (p + 15) >> 4;
    w_hi = (p + d.n) >> 4;
    if (w_hi < w_lo) w_hi = w_lo;
}

template <int Q>
__device__ __forceinline__ void bulk_pass(const u8 *src, u64 p, u64 w_lo, u64 words, u64 k0, u32 r)
{
    uint4 lo[BULK_WORDS], hi[BULK_WORDS];
#pragma unroll
    for (int i = 0; i < BULK_WORDS; ++i) {
        const u64 k = k0 + (u64)i * BULK_THREADS;
        if (k < words) {
            // destination word (w_lo + k) holds payload bytes from (w_lo + k) * 16 - p on; the source is 16-aligned
            const u64 s = (u64)(uintptr_t)src + (w_lo + k) * 16 - p;
            const uint4 *s16 = (const uint4 *)(uintptr_t)(s & ~(u64)15);
            lo[i] = s16[0];
            if (Q != 0 || r != 0) hi[i] = s16[1];
        }
    }
#pragma unroll
    for (int i = 0; i < BULK_WORDS; ++i) {
        const u64 k = k0 + (u64)i * BULK_THREADS;
        if (k < words) {
            uint4 *d16 = (uint4 *)(uintptr_t)((w_lo + k) * 16);
            *d16 = (Q == 0 && r == 0) ? lo[i] : shift_words<Q>(lo[i], hi[i], r);
        }
    }
}

// grid: x = chunks of BULK_CHUNK_WORDS words (host bound from the capacities), y = block
__global__ __launch_bounds__(BULK_THREADS) void pack_bulk(const PackDesc *__restrict__ desc, const u32 *__restrict__ verdict)
{
    if (*verdict == 0) return;
    const PackDesc d = desc[blockIdx.y];
    u64 w_lo, w_hi;
    whole_words(d, w_lo, w_hi);
    const u64 words = w_hi - w_lo;
    const u64 c0 = (u64)blockIdx.x * BULK_CHUNK_WORDS;
    if (c0 >= words) return;
    const u64 p = (u64)(uintptr_t)(d.dst + d.hdr_len);
    const u32 m = (u32)((0u - (u32)p) & 15u);        // (src - dst) mod 16, the block's constant misalignment
    const u32 q = m >> 2, r = m & 3u;
    for (int pass = 0; pass < BULK_PASSES; ++pass) {
        const u64 k0 = c0 + (u64)pass * BULK_THREADS * BULK_WORDS + threadIdx.x;
        switch (q) {                                 // uniform per workgroup
        case 0: bulk_pass<0>(d.src, p, w_lo, words, k0, r); break;
        case 1: bulk_pass<1>(d.src, p, w_lo, words, k0, r); break;
        case 2: bulk_pass<2>(d.src, p, w_lo, words, k0, r); break;
        default: bulk_pass<3>(d.src, p, w_lo, words, k0, r); break;
        }
    }
}

// a lane per block: the block's "@size@" and the payload bytes outside its whole words; lane 0 of block 0 also the file's
// prefix (`head`, head_len bytes at the file's start)
__global__ __launch_bounds__(64) void pack_seams(const PackDesc *__restrict__ desc, int nblocks, const u32 *__restrict__ verdict,
                                                 u8 *dst, u64 nblk_hdr, u32 head_len)
{
    if (*verdict == 0) return;
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b == 0 && head_len) {
        dst[0] = '@';
        put_dec(dst + 1, nblk_hdr);
    }
    if (b >= nblocks) return;
    const PackDesc d = desc[b];
    u8 *o = d.dst;
    if (d.hdr_len) {
        *o++ = '@';
        o = put_dec(o, d.hdr_val);
        *o++ = '@';
    }
    u64 w_lo, w_hi;
    whole_words(d, w_lo, w_hi);
    const u64 p = (u64)(uintptr_t)o, e = p + d.n;
    const u64 head_end = w_hi == w_lo ? e : w_lo * 16;         // no whole word: every byte is the seam's
    for (u64 a = p; a < head_end; ++a) *(u8 *)(uintptr_t)a = d.src[a - p];
    if (w_hi > w_lo)
        for (u64 a = w_hi * 16; a < e; ++a) *(u8 *)(uintptr_t)a = d.src[a - p];
}

// ---- text: .cod and .freq --------------------------------------------------------------------------------------------
// field length of symbol s: its code's length (.cod); the digits of its count where the count differs from the symbol
// before it, else 0 (.freq, f.c:89-119: a run of equal counts prints its value once)
struct CodText {
    const shafa_code_table *t;
    __device__ u32 len(int b, int s) const { return t[b].len[s]; }
    __device__ void put(int b, int s, u8 *p) const
    {
        const shafa_code_table &tb = t[b];
        const u32 n = tb.len[s];
        for (u32 i = 0; i < n; ++i) p[i] = (u8)('0' + ((tb.bits[s][i >> 3] >> (7 - (i & 7))) & 1));
    }
};
struct FreqText {
    const u64 *f;
    __device__ u32 len(int b, int s) const
    {
        const u64 *fb = f + (size_t)b * 256;
        return (s == 0 || fb[s] != fb[s - 1]) ? dec_digits(fb[s]) : 0u;
    }
    __device__ void put(int b, int s, u8 *p) const
    {
        const u64 *fb = f + (size_t)b * 256;
        if (s == 0 || fb[s] != fb[s - 1]) put_dec(p, fb[s]);
    }
};

// 256 lanes: the block's field offsets (exclusive, separators included) and its text length
__device__ inline u32 field_scan(u32 flen, u32 *wsum32, u32 *total)
{
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const u32 v = flen + (tid != 255 ? 1u : 0u);     // 255 separators
    const u32 incl = dpp_scan_add(v);
    if (lane == 63) wsum32[wv] = incl;
    __syncthreads();
    u32 base = 0;
    for (u32 w = 0; w < wv; ++w) base += wsum32[w];
    *total = wsum32[0] + wsum32[1] + wsum32[2] + wsum32[3];
    return base + incl - v;
}

template <typename Text>
__global__ __launch_bounds__(256) void pack_measure(Text tx, u64 *__restrict__ body)
{
    __shared__ u32 wsum32[4];
    const int b = blockIdx.x;
    u32 total;
    (void)field_scan(tx.len(b, (int)threadIdx.x), wsum32, &total);
    if (threadIdx.x == 0) body[b] = total;
}

// block b's frame at its descriptor: "@<size>@" + fields
template <typename Text>
__device__ __forceinline__ void text_frame(const Text &tx, int b, const PackDesc &d)
{
    __shared__ u32 wsum32[4];
    const int s = (int)threadIdx.x;
    u32 total;
    const u32 off = field_scan(tx.len(b, s), wsum32, &total);
    u8 *body = d.dst + d.hdr_len;
    tx.put(b, s, body + off);
    if (s != 255) body[off + tx.len(b, s)] = ';';
    if (s == 0) {
        u8 *o = d.dst;
        *o++ = '@';
        o = put_dec(o, d.hdr_val);
        *o = '@';
    }
}

// block b's frame; block 0 also the file's head "@<mode>@<n>", the last block the file's "@0"
template <typename Text>
__global__ __launch_bounds__(256) void pack_text(Text tx, const PackDesc *__restrict__ desc, int nblocks,
                                                 const u32 *__restrict__ verdict, u8 *dst, char mode)
{
    if (*verdict == 0) return;
    const int b = blockIdx.x, s = (int)threadIdx.x;
    const PackDesc d = desc[b];
    text_frame(tx, b, d);
    if (s == 1 && b == 0) {
        dst[0] = '@';
        dst[1] = (u8)mode;
        dst[2] = '@';
        put_dec(dst + 3, (u64)nblocks);
    }
    if (s == 2 && b == nblocks - 1) {
        u8 *e = d.dst + d.hdr_len + d.n;
        e[0] = '@';
        e[1] = '0';
    }
}

// workspace: [verdict: 16 B][descriptors][text lengths]
struct PackWs {
    u32 *verdict;
    PackDesc *desc;
    u64 *body;
};

int pack_ws(Batch *bt, hipStream_t st, int nblocks, PackWs &w)
{
    const size_t o_desc = 256, o_body = o_desc + (size_t)nblocks * sizeof(PackDesc);
    const size_t bytes = o_body + (size_t)nblocks * 8;
    if (int rc = batch_reserve(bt, st, bytes)) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    w.verdict = (u32 *)ws;
    w.desc = (PackDesc *)(ws + o_desc);
    w.body = (u64 *)(ws + o_body);
    return SHAFA_SUCCESS;
}

PlanBlocks plan_blocks(u32 hdr, const PackSrc *srcs, const u64 *n, const u64 *hdr_vals, PackDesc *desc, u32 *verdict, int *err)
{
    PlanBlocks p = {};
    p.hdr = hdr;
    p.srcs = srcs;
    p.n = n;
    p.hdr_vals = hdr_vals;
    p.desc = desc;
    p.verdict = verdict;
    p.err = err;
    return p;
}

// pack_bulk's grid x: the chunks of the largest of nb payload regions
int bulk_chunks(int nb, const u64 *h_src_cap, u64 &max_chunks)
{
    max_chunks = 1;
    for (int b = 0; b < nb; ++b) {
        const u64 c = ceil_div_u64(h_src_cap[b] / 16 + 1, BULK_CHUNK_WORDS);
        if (c > max_chunks) max_chunks = c;
    }
    return max_chunks > 0x7FFFFFFFull ? SHAFA_LACK_OF_MEMORY : SHAFA_SUCCESS;
}

void stage_srcs(PackSrc *hp, int nb, const u8 *d_src, const u64 *h_src_off, const u64 *h_src_cap)
{
    for (int b = 0; b < nb; ++b) {
        hp[b].src = d_src + h_src_off[b];
        hp[b].cap = h_src_cap[b];
    }
}

template <typename Text>
int text_launch(Batch *bt, hipStream_t st, int nblocks, char mode, const u64 *d_sizes, Text tx, u8 *d_dst, u64 dst_cap,
                u64 *d_dst_n)
{
    if (nblocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    PackWs w;
    if (int rc = pack_ws(bt, st, nblocks, w)) return rc;
    hipLaunchKernelGGL(pack_measure<Text>, dim3((u32)nblocks), dim3(256), 0, st, tx, w.body);
    PlanArgs a = {};
    a.blk = plan_blocks(1, nullptr, w.body, d_sizes, w.desc, w.verdict, bt->d_err);
    a.nblocks = nblocks;
    a.head_len = 3 + dec_digits((u64)nblocks);       // "@<mode>@<n>"
    a.tail_len = 2;                                  // "@0"
    a.dst = d_dst;
    a.dst_cap = dst_cap;
    a.dst_n = d_dst_n;
    hipLaunchKernelGGL(pack_plan, dim3(1), dim3(PLAN_THREADS), 0, st, a);
    hipLaunchKernelGGL(pack_text<Text>, dim3((u32)nblocks), dim3(256), 0, st, tx, (const PackDesc *)w.desc, nblocks,
                       (const u32 *)w.verdict, d_dst, mode);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

int payload_launch(Batch *bt, hipStream_t st, int nblocks, int framing, const u8 *d_src, const u64 *h_src_off,
                   const u64 *h_src_cap, const u64 *d_src_n, u8 *d_dst, u64 dst_cap, u64 *d_dst_n)
{
    if (nblocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    PackWs w;
    if (int rc = pack_ws(bt, st, nblocks, w)) return rc;
    u64 max_chunks;
    if (int rc = bulk_chunks(nblocks, h_src_cap, max_chunks)) return rc;
    const size_t par_bytes = (size_t)nblocks * sizeof(PackSrc);
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    PackSrc *hp = (PackSrc *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    stage_srcs(hp, nblocks, d_src, h_src_off, h_src_cap);
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    const bool shaf = framing == SHAFA_FRAME_SHAF;
    PlanArgs a = {};
    a.blk = plan_blocks(shaf ? 1u : 0u, (const PackSrc *)dpar, d_src_n, nullptr, w.desc, w.verdict, bt->d_err);
    a.nblocks = nblocks;
    a.head_len = shaf ? 1 + dec_digits((u64)nblocks) : 0;     // "@<n>"
    a.tail_len = 0;
    a.dst = d_dst;
    a.dst_cap = dst_cap;
    a.dst_n = d_dst_n;
    hipLaunchKernelGGL(pack_plan, dim3(1), dim3(PLAN_THREADS), 0, st, a);
    hipLaunchKernelGGL(pack_bulk, dim3((u32)max_chunks, (u32)nblocks), dim3(BULK_THREADS), 0, st, (const PackDesc *)w.desc,
                       (const u32 *)w.verdict);
    hipLaunchKernelGGL(pack_seams, dim3((u32)ceil_div_u64((u64)nblocks, 64)), dim3(64), 0, st, (const PackDesc *)w.desc, nblocks,
                       (const u32 *)w.verdict, d_dst, (u64)nblocks, (u32)a.head_len);
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

// ---- segmented packs: many files in one launch sequence ----------------------------------------------------------------
// File f is blocks first .. first + count - 1 of the call's block arrays; its frames take the descriptor slots slot ..
// slot + count - 1 (a block listed by two files has a slot in each).  Per file: a verdict word (1: write it) and its length.
// The movers' global verdict word stays 1: a refused file's descriptors are rewritten to n = 0, hdr_len = 0, for which the
// unchanged pack_bulk / pack_seams write nothing (unpack.hip's rule for a refused block).
struct FileRec {
    u8 *dst;
    u64 cap;
    int first, count;
    u32 slot;
    u32 mode;                // text: 'R' / 'N'
};

struct FilesPlanArgs {
    PlanBlocks blk;          // desc: per slot; verdict: 1
    const FileRec *files;
    u32 head;                // the file's prefix: 0 none, 1 "@<n>", 2 "@<mode>@<n>"
    u64 tail_len;            // "@0": 2, else 0
    u64 *dst_n;              // per file
    u32 *slot_file;          // per slot: its file
    u32 *fverdict;           // per file
};

__device__ inline u64 file_head_len(u32 head, int count)
{
    return head == 0 ? 0 : (head == 1 ? 1u : 3u) + dec_digits((u64)count);
}

// one workgroup per file: pack_plan's scan and checks over the file's blocks
__global__ __launch_bounds__(PLAN_THREADS) void pack_file_plan(FilesPlanArgs a)
{
    __shared__ u32 go_sh;
    const u32 tid = threadIdx.x, f = blockIdx.x;
    const FileRec fr = a.files[f];
    PackDesc *desc = a.blk.desc + fr.slot;
    const u32 go = plan_frames(a.blk, fr.first, fr.count, desc, fr.dst, fr.cap, file_head_len(a.head, fr.count), a.tail_len,
                               a.dst_n + f, a.blk.err + fr.first);
    if (tid == 0) {
        go_sh = go;
        a.fverdict[f] = go;
        if (f == 0) *a.blk.verdict = 1;
    }
    __syncthreads();
    for (int i = (int)tid; i < fr.count; i += PLAN_THREADS) {      // each lane: the slots it wrote in plan_frames
        a.slot_file[fr.slot + i] = f;
        if (!go_sh) {
            desc[i].n = 0;
            desc[i].hdr_len = 0;
        }
    }
}

// a lane per file: its prefix ("@<n>" / "@<mode>@<n>") and, for text, its "@0"
__global__ __launch_bounds__(64) void pack_file_ends(const FileRec *__restrict__ files, int nfiles, const u32 *__restrict__ fverdict,
                                                     const u64 *__restrict__ dst_n, u32 head, u32 tail)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= nfiles || fverdict[f] == 0) return;
    const FileRec fr = files[f];
    u8 *o = fr.dst;
    if (head) {
        *o++ = '@';
        if (head == 2) {
            *o++ = (u8)fr.mode;
            *o++ = '@';
        }
        put_dec(o, (u64)fr.count);
    }
    if (tail) {
        u8 *e = fr.dst + dst_n[f] - 2;
        e[0] = '@';
        e[1] = '0';
    }
}

// pack_text without the file's head and tail: slot i's "@<size>@" + fields, when its file was not refused
template <typename Text>
__global__ __launch_bounds__(256) void pack_file_text(Text tx, const PackDesc *__restrict__ desc, const FileRec *__restrict__ files,
                                                      const u32 *__restrict__ slot_file, const u32 *__restrict__ fverdict)
{
    const u32 i = blockIdx.x, f = slot_file[i];
    if (fverdict[f] == 0) return;
    const FileRec fr = files[f];
    text_frame(tx, fr.first + (int)(i - fr.slot), desc[i]);
}

// the host's view of a segmented call: the blocks it reads ([0, nb)) and its descriptor slots
struct FilesShape {
    int nb;
    u32 slots;
};

// argument checks shared by the three entries (no HIP call)
int files_check(const Batch *bt, int nfiles, const int *h_first, const int *h_count, const u64 *h_dst_off,
                const u64 *h_dst_cap, const char *h_modes, FilesShape &sh)
{
    if (!bt || nfiles < 1 || !h_first || !h_count || !h_dst_off || !h_dst_cap) return SHAFA_OUTSIDE_MODULE;
    long long slots = 0, nb = 0;
    for (int f = 0; f < nfiles; ++f) {
        const long long first = h_first[f], count = h_count[f];
        if (count < 1 || first < 0 || first + count > bt->max_blocks) return SHAFA_OUTSIDE_MODULE;
        if (h_modes && h_modes[f] != 'R' && h_modes[f] != 'N') return SHAFA_OUTSIDE_MODULE;
        slots += count;
        if (first + count > nb) nb = first + count;
    }
    if (slots > 0x7FFFFFFFll) return SHAFA_LACK_OF_MEMORY;
    sh.nb = (int)nb;
    sh.slots = (u32)slots;
    return SHAFA_SUCCESS;
}

// workspace: [verdict: 256 B][file verdicts][descriptors][text lengths][slot files]
struct FilesWs {
    u32 *verdict, *fverdict;
    PackDesc *desc;
    u64 *body;
    u32 *slot_file;
};

size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

int files_ws(Batch *bt, hipStream_t st, int nfiles, const FilesShape &sh, FilesWs &w)
{
    const size_t o_desc = 256 + al16((size_t)nfiles * 4), o_body = o_desc + (size_t)sh.slots * sizeof(PackDesc);
    const size_t o_slot = o_body + al16((size_t)sh.nb * 8);
    if (int rc = batch_reserve(bt, st, o_slot + (size_t)sh.slots * 4)) return rc;
    u8 *ws = (u8 *)bt->d_ws;
    w.verdict = (u32 *)ws;
    w.fverdict = (u32 *)(ws + 256);
    w.desc = (PackDesc *)(ws + o_desc);
    w.body = (u64 *)(ws + o_body);
    w.slot_file = (u32 *)(ws + o_slot);
    return SHAFA_SUCCESS;
}

// the file records (and, for payloads, the blocks' sources after them) in the staging of the launch's parameters
void files_records(FileRec *hp, int nfiles, const int *h_first, const int *h_count, const char *h_modes, u8 *d_dst,
                   const u64 *h_dst_off, const u64 *h_dst_cap)
{
    u32 slot = 0;
    for (int f = 0; f < nfiles; ++f) {
        hp[f].dst = d_dst + h_dst_off[f];
        hp[f].cap = h_dst_cap[f];
        hp[f].first = h_first[f];
        hp[f].count = h_count[f];
        hp[f].slot = slot;
        hp[f].mode = h_modes ? (u32)(u8)h_modes[f] : 0u;
        slot += (u32)h_count[f];
    }
}

template <typename Text>
int text_files_launch(Batch *bt, hipStream_t st, int nfiles, const FilesShape &sh, const int *h_first, const int *h_count,
                      const char *h_modes, const u64 *d_sizes, Text tx, u8 *d_dst, const u64 *h_dst_off, const u64 *h_dst_cap,
                      u64 *d_dst_n)
{
    FilesWs w;
    if (int rc = files_ws(bt, st, nfiles, sh, w)) return rc;
    const size_t par_bytes = (size_t)nfiles * sizeof(FileRec);
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    FileRec *hp = (FileRec *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    files_records(hp, nfiles, h_first, h_count, h_modes, d_dst, h_dst_off, h_dst_cap);
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    const FileRec *d_files = (const FileRec *)dpar;
    hipLaunchKernelGGL(pack_measure<Text>, dim3((u32)sh.nb), dim3(256), 0, st, tx, w.body);
    FilesPlanArgs a = {};
    a.blk = plan_blocks(1, nullptr, w.body, d_sizes, w.desc, w.verdict, bt->d_err);
    a.files = d_files;
    a.head = 2;                                      // "@<mode>@<n>"
    a.tail_len = 2;                                  // "@0"
    a.dst_n = d_dst_n;
    a.slot_file = w.slot_file;
    a.fverdict = w.fverdict;
    hipLaunchKernelGGL(pack_file_plan, dim3((u32)nfiles), dim3(PLAN_THREADS), 0, st, a);
    hipLaunchKernelGGL(pack_file_text<Text>, dim3(sh.slots), dim3(256), 0, st, tx, (const PackDesc *)w.desc, d_files,
                       (const u32 *)w.slot_file, (const u32 *)w.fverdict);
    hipLaunchKernelGGL(pack_file_ends, dim3((u32)ceil_div_u64((u64)nfiles, 64)), dim3(64), 0, st, d_files, nfiles,
                       (const u32 *)w.fverdict, (const u64 *)d_dst_n, 2u, 1u);
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

int payload_files_launch(Batch *bt, hipStream_t st, int nfiles, const FilesShape &sh, const int *h_first, const int *h_count,
                         int framing, const u8 *d_src, const u64 *h_src_off, const u64 *h_src_cap, const u64 *d_src_n, u8 *d_dst,
                         const u64 *h_dst_off, const u64 *h_dst_cap, u64 *d_dst_n)
{
    u64 max_chunks;
    if (int rc = bulk_chunks(sh.nb, h_src_cap, max_chunks)) return rc;
    int max_y = 0;
    HIP_TRY(hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, bt->device));
    if (max_y < 1) max_y = 1;
    FilesWs w;
    if (int rc = files_ws(bt, st, nfiles, sh, w)) return rc;
    const size_t o_src = (size_t)nfiles * sizeof(FileRec), par_bytes = o_src + (size_t)sh.nb * sizeof(PackSrc);
    u8 *dpar = batch_params_begin(bt, par_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    FileRec *hp = (FileRec *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, par_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    files_records(hp, nfiles, h_first, h_count, nullptr, d_dst, h_dst_off, h_dst_cap);
    stage_srcs((PackSrc *)((u8 *)hp + o_src), sh.nb, d_src, h_src_off, h_src_cap);
    if (int rc = batch_params_commit(bt, st, hp, par_bytes)) return rc;
    const FileRec *d_files = (const FileRec *)dpar;
    const bool shaf = framing == SHAFA_FRAME_SHAF;
    FilesPlanArgs a = {};
    a.blk = plan_blocks(shaf ? 1u : 0u, (const PackSrc *)(dpar + o_src), d_src_n, nullptr, w.desc, w.verdict, bt->d_err);
    a.files = d_files;
    a.head = shaf ? 1u : 0u;                         // "@<n>"
    a.tail_len = 0;
    a.dst_n = d_dst_n;
    a.slot_file = w.slot_file;
    a.fverdict = w.fverdict;
    hipLaunchKernelGGL(pack_file_plan, dim3((u32)nfiles), dim3(PLAN_THREADS), 0, st, a);
    // the bulk grid puts slots on y: in slices of at most the device's grid height
    for (u32 s0 = 0; s0 < sh.slots; s0 += (u32)max_y) {
        const u32 ns = sh.slots - s0 < (u32)max_y ? sh.slots - s0 : (u32)max_y;
        hipLaunchKernelGGL(pack_bulk, dim3((u32)max_chunks, ns), dim3(BULK_THREADS), 0, st, (const PackDesc *)(w.desc + s0),
                           (const u32 *)w.verdict);
    }
    hipLaunchKernelGGL(pack_seams, dim3((u32)ceil_div_u64((u64)sh.slots, 64)), dim3(64), 0, st, (const PackDesc *)w.desc,
                       (int)sh.slots, (const u32 *)w.verdict, (u8 *)nullptr, (u64)0, (u32)0);
    if (shaf)
        hipLaunchKernelGGL(pack_file_ends, dim3((u32)ceil_div_u64((u64)nfiles, 64)), dim3(64), 0, st, d_files, nfiles,
                           (const u32 *)w.fverdict, (const u64 *)d_dst_n, 1u, 0u);
    HIP_TRY(hipGetLastError());
    return pscope.done();
}

}  // namespace

static_assert(sizeof(FileRec) == 32, "file records keep the blocks' PackSrc records after them 16-aligned");
static_assert(sizeof(MoveDesc) == sizeof(PackDesc) && offsetof(MoveDesc, src) == offsetof(PackDesc, src) &&
                  offsetof(MoveDesc, dst) == offsetof(PackDesc, dst) && offsetof(MoveDesc, n) == offsetof(PackDesc, n) &&
                  offsetof(MoveDesc, hdr_len) == offsetof(PackDesc, hdr_len),
              "MoveDesc (internal.hpp) is PackDesc's layout");

int pack_move_launch(hipStream_t st, int nblocks, const MoveDesc *d_bulk, const MoveDesc *d_seam, const u32 *d_verdict,
                     u64 max_n)
{
    const u64 chunks = ceil_div_u64(max_n / 16 + 2, BULK_CHUNK_WORDS);
    if (chunks > 0x7FFFFFFFull) return SHAFA_LACK_OF_MEMORY;
    hipLaunchKernelGGL(pack_bulk, dim3((u32)chunks, (u32)nblocks), dim3(BULK_THREADS), 0, st, (const PackDesc *)d_bulk, d_verdict);
    hipLaunchKernelGGL(pack_seams, dim3((u32)ceil_div_u64((u64)nblocks, 64)), dim3(64), 0, st, (const PackDesc *)d_seam, nblocks,
                       d_verdict, (u8 *)nullptr, (u64)0, (u32)0);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

extern "C" {

size_t shafa_hip_pack_payloads_max(int nblocks, const uint64_t *h_src_cap, int framing)
{
    if (nblocks < 1 || !h_src_cap || (framing != SHAFA_FRAME_RAW && framing != SHAFA_FRAME_SHAF)) return 0;
    size_t n = framing == SHAFA_FRAME_SHAF ? 1 + dec_digits((u64)nblocks) : 0;
    for (int b = 0; b < nblocks; ++b) n += h_src_cap[b] + (framing == SHAFA_FRAME_SHAF ? 2 + dec_digits(h_src_cap[b]) : 0);
    return n;
}

size_t shafa_hip_pack_cod_max(int nblocks)
{
    if (nblocks < 1) return 0;
    return 3 + dec_digits((u64)nblocks) + (size_t)nblocks * (22 + 256 * 255 + 255) + 2;
}

size_t shafa_hip_pack_freq_max(int nblocks)
{
    if (nblocks < 1) return 0;
    return 3 + dec_digits((u64)nblocks) + (size_t)nblocks * (22 + 256 * 20 + 255) + 2;
}

int shafa_hipd_pack_payloads(shafa_hipd_batch *b, void *stream, int nblocks, int framing, const uint8_t *d_src,
                             const uint64_t *h_src_off, const uint64_t *h_src_cap, const uint64_t *d_src_n, uint8_t *d_dst,
                             uint64_t dst_cap, uint64_t *d_dst_n)
{
    if (!b || !d_src || !h_src_off || !h_src_cap || !d_src_n || !d_dst || !d_dst_n || nblocks < 1) return SHAFA_OUTSIDE_MODULE;
    if (framing != SHAFA_FRAME_RAW && framing != SHAFA_FRAME_SHAF) return SHAFA_OUTSIDE_MODULE;
    if ((uintptr_t)d_src & 15) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (h_src_off[i] & 15) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return payload_launch((Batch *)b, (hipStream_t)stream, nblocks, framing, d_src, h_src_off, h_src_cap, d_src_n, d_dst,
                          dst_cap, d_dst_n);
}

int shafa_hipd_pack_cod(shafa_hipd_batch *b, void *stream, int nblocks, char mode, const uint64_t *d_sizes,
                        const shafa_code_table *d_tables, uint8_t *d_dst, uint64_t dst_cap, uint64_t *d_dst_n)
{
    if (!b || !d_sizes || !d_tables || !d_dst || !d_dst_n || nblocks < 1 || (mode != 'R' && mode != 'N'))
        return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return text_launch((Batch *)b, (hipStream_t)stream, nblocks, mode, d_sizes, CodText{d_tables}, d_dst, dst_cap, d_dst_n);
}

int shafa_hipd_pack_freq(shafa_hipd_batch *b, void *stream, int nblocks, char mode, const uint64_t *d_sizes,
                         const uint64_t *d_freq, uint8_t *d_dst, uint64_t dst_cap, uint64_t *d_dst_n)
{
    if (!b || !d_sizes || !d_freq || !d_dst || !d_dst_n || nblocks < 1 || (mode != 'R' && mode != 'N'))
        return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return text_launch((Batch *)b, (hipStream_t)stream, nblocks, mode, d_sizes, FreqText{d_freq}, d_dst, dst_cap, d_dst_n);
}

int shafa_hipd_pack_payloads_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                                   int framing, const uint8_t *d_src, const uint64_t *h_src_off, const uint64_t *h_src_cap,
                                   const uint64_t *d_src_n, uint8_t *d_dst, const uint64_t *h_dst_off,
                                   const uint64_t *h_dst_cap, uint64_t *d_dst_n)
{
    if (!d_src || !h_src_off || !h_src_cap || !d_src_n || !d_dst || !d_dst_n) return SHAFA_OUTSIDE_MODULE;
    if (framing != SHAFA_FRAME_RAW && framing != SHAFA_FRAME_SHAF) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    FilesShape sh;
    if (int rc = files_check(bt, nfiles, h_first, h_count, h_dst_off, h_dst_cap, nullptr, sh)) return rc;
    for (int f = 0; f < nfiles; ++f)
        for (int i = h_first[f]; i < h_first[f] + h_count[f]; ++i)
            if ((uintptr_t)(d_src + h_src_off[i]) & 15) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return payload_files_launch(bt, (hipStream_t)stream, nfiles, sh, h_first, h_count, framing, d_src, h_src_off, h_src_cap,
                                d_src_n, d_dst, h_dst_off, h_dst_cap, d_dst_n);
}

int shafa_hipd_pack_cod_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                              const char *h_modes, const uint64_t *d_sizes, const shafa_code_table *d_tables,
                              uint8_t *d_dst, const uint64_t *h_dst_off, const uint64_t *h_dst_cap, uint64_t *d_dst_n)
{
    if (!h_modes || !d_sizes || !d_tables || !d_dst || !d_dst_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    FilesShape sh;
    if (int rc = files_check(bt, nfiles, h_first, h_count, h_dst_off, h_dst_cap, h_modes, sh)) return rc;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_files_launch(bt, (hipStream_t)stream, nfiles, sh, h_first, h_count, h_modes, d_sizes, CodText{d_tables}, d_dst,
                             h_dst_off, h_dst_cap, d_dst_n);
}

int shafa_hipd_pack_freq_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                               const char *h_modes, const uint64_t *d_sizes, const uint64_t *d_freq,
                               uint8_t *d_dst, const uint64_t *h_dst_off, const uint64_t *h_dst_cap, uint64_t *d_dst_n)
{
    if (!h_modes || !d_sizes || !d_freq || !d_dst || !d_dst_n) return SHAFA_OUTSIDE_MODULE;
    Batch *bt = (Batch *)b;
    FilesShape sh;
    if (int rc = files_check(bt, nfiles, h_first, h_count, h_dst_off, h_dst_cap, h_modes, sh)) return rc;
    if (int rc = batch_enter(bt, (hipStream_t)stream)) return rc;
    return text_files_launch(bt, (hipStream_t)stream, nfiles, sh, h_first, h_count, h_modes, d_sizes, FreqText{d_freq}, d_dst,
                             h_dst_off, h_dst_cap, d_dst_n);
}

}  // extern "C"
