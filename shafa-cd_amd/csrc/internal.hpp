// internal.hpp — structures shared between the C-ABI layer (api.hip) and the kernel launchers.
#pragma once

#include "common.hpp"

#include <string.h>
#include <vector>

// one region of the pinned staging ring: [off, off + bytes), read by copies enqueued on `st`; `ev` is recorded on
// `st` when the next region is handed out (or at finish), i.e. after those copies
struct StageSeg {
    size_t off, bytes;
    hipStream_t st;
    hipEvent_t ev;
    bool sealed;
};

// Reusable per-batch context behind the opaque shafa_hipd_batch handle.
// parameter uploads of at most this many bytes go into the launch's stream (api.hip, batch_params_commit)
constexpr size_t PARAMS_INLINE_BYTES = 64 * 1024;

struct Batch {
    int device;            // the device the batch was created on: its workspace, error words and kernels live there
    hipStream_t last_st;   // the stream of the batch's last launch (a batch serves ONE stream at a time: a launch on a
    bool has_last;         //   different stream first waits for the previous one, see batch_enter)
    int max_blocks;
    size_t max_block_bytes;
    void *d_ws;            // device workspace (grow-only; grown outside timed regions by warm-up calls)
    size_t ws_bytes;
    u8 *h_stage;           // pinned host staging ring for parameter blocks / tables: every region handed out is
    size_t stage_bytes;    //   fenced by an event recorded on the stream that copies from it; a region is reused only
    size_t stage_used;     //   after ITS event (no device-wide synchronisation on the enqueue path)
    std::vector<StageSeg> *segs;
    void *d_par_hist;      // max_blocks * 48 B of hist256 parameters (separate from d_ws: hist256 may
                           //   run right after another op that still owns the workspace)
    int *d_err;            // one error code per block (first error wins)
    int *h_err;            // pinned mirror
    int *h_hosterr;        // errors found on the host while preparing a launch (malformed tables)
    // Parameter records and code tables of a launch travel on a SIDE stream into one of two device buffers, so that the
    // copy (and its hand-over between the copy engine and the compute queue, ~50-100 us either way) overlaps the kernels of
    // the launch before instead of sitting between two launches: batch_params_begin / _commit / _done.
    hipStream_t copy_st;
    void *d_par[2];
    size_t par_bytes[2];
    hipEvent_t par_ready[2], par_free[2];
    bool par_used[2];
    int par_turn, par_cur;
    bool par_inline;            // this launch's parameters are copied in the launch's own stream (few blocks), not on copy_st
    bool par_dma;               // the batch belongs to a pipe slot: parameters by hipMemcpyAsync on the side stream (api.hip)
};

// Every layer-2 entry point starts with this: checks that the calling thread's current device is the batch's, and
// serialises a change of stream (the workspace, the error words and the staging ring are shared by all launches of
// a batch, so work enqueued on another stream must have finished before the new stream's launch reuses them).
int batch_enter(Batch *b, hipStream_t st);
// shafa_hipd_finish, telling a failure of the call (stream / copy error: no block has a result, every block_err = the code)
// from the first block's error
int batch_finish(Batch *b, hipStream_t st, int nblocks, int *h_block_err, bool *call_failed);

// RAII: make `device` current for the calling thread, restore the caller's device on exit (a torch caller, or layer 1
// next to a multi-device pipe, must not see its current device change under it)
struct DeviceGuard {
    int prev;
    bool changed;
    explicit DeviceGuard(int device) : prev(-1), changed(false)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) changed = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// make sure the device workspace holds `bytes` (growing waits for `st`, the only stream that uses this batch's workspace)
int batch_reserve(Batch *b, hipStream_t st, size_t bytes);
// hand out `bytes` of the pinned staging ring for copies that the caller enqueues on `st`
void *batch_stage(Batch *b, hipStream_t st, size_t bytes);
// every copy enqueued on `st` so far has completed (the caller synchronised `st`): release its regions
void batch_stage_retire(Batch *b, hipStream_t st);

// Parameters of a launch (records + tables), uploaded off the launch stream:
//   d = batch_params_begin(b, bytes)          the device buffer the launch's parameters will live in (records may point into it)
//   hs = batch_stage(b, b->copy_st, bytes)    pinned staging, filled by the caller
//   batch_params_commit(b, st, hs, bytes)     copy on the side stream (after the kernels that last read this buffer); `st` waits for it
//   ... kernels on `st` ...
//   batch_params_done(b, st)                  the buffer is free again once these kernels have run
u8 *batch_params_begin(Batch *b, size_t bytes);
int batch_upload(Batch *b, hipStream_t st, void *dst, const void *src, size_t bytes);
int batch_params_commit(Batch *b, hipStream_t st, const void *hs, size_t bytes);
int batch_params_done(Batch *b, hipStream_t st);
// A launcher's early `return rc` after batch_params_begin must still mark the buffer's last reader: kernels already enqueued
// may be reading it, and the next launch that gets this buffer waits on par_free before it overwrites it.
struct ParamsScope {
    Batch *b;
    hipStream_t st;
    bool open;
    ParamsScope(Batch *b_, hipStream_t st_) : b(b_), st(st_), open(true) {}
    ~ParamsScope() { if (open) (void)batch_params_done(b, st); }
    int done() { open = false; return batch_params_done(b, st); }
    ParamsScope(const ParamsScope &) = delete;
    ParamsScope &operator=(const ParamsScope &) = delete;
};

// the offset of the next `bytes` of an upload whose parts start at multiples of 16
inline size_t take16(size_t &pos, size_t bytes)
{
    const size_t at = pos;
    pos = (pos + bytes + 15) & ~(size_t)15;
    return at;
}

// ---- the host set-up of a tile-walk launch (api.hip) -------------------------------------------
// A launcher whose kernels walk the tiles of the blocks' capacities (tile_pass.hpp's TpWalk, seek.hip's spans) gets from
// tile_setup, in the batch's workspace,
//     [scratch: scratch_per_tile bytes per tile + scratch_fixed, for the kernels][offsets][capacities][extras ...][tbase]
// every part at a multiple of 16 bytes and zero padded to the next; all but the scratch is put together in pinned staging and
// uploaded in ONE batch_upload on `st`.  tbase[b] is the number of block b's first tile among the tiles of all blocks, nblocks + 1
// entries of 32 bits; `unit` is the tile: TP_TILE bytes, elements or records, or the span.  An extra is a host array of the
// caller's that its kernels read behind the capacities (NULL: zeros).
// Returns SHAFA_LACK_OF_MEMORY for 2^31 tiles or more (tile_count) before anything is touched, then what batch_reserve,
// batch_stage (SHAFA_LACK_OF_MEMORY) and batch_upload return.
constexpr u32 TP_MAX_WGS = 16384;                  // a tile walk's workgroups per launch (64 a CU, 8 of them resident at a time)
constexpr int TILE_EXTRAS = 3;
struct TileExtra {
    const void *h;
    size_t bytes;
};
struct TileSetup {
    const u64 *off, *cap;          // device pointers into the workspace
    const u32 *tbase;
    const u8 *extra[TILE_EXTRAS];
    u8 *scratch;
    u32 nt;                        // the tiles of all blocks
    u32 per_wg, wgs;               // equal runs of tiles over at most TP_MAX_WGS workgroups (per_wg >= 1; no tile: no workgroup);
                                   //   a launcher with a grid rule of its own takes nt alone
};
int tile_setup(Batch *bt, hipStream_t st, int nblocks, const u64 *h_off, const u64 *h_cap, u32 unit, const TileExtra *extras,
               int nextras, size_t scratch_per_tile, size_t scratch_fixed, TileSetup *s);
// the first block at which the capacities' tiles of `unit` number 2^31 or more (the kernels number them in 31 bits), nblocks
// where they stay below; *ntiles (where asked for) is then their number
int tile_count(int nblocks, const u64 *h_cap, u64 unit, u64 *ntiles = nullptr);

// ---- the grids of the two RLE launch chains (rle_decode.hip, rle_encode.hip) -------
// Both put (rows of the largest block) x (blocks) workgroups of 256 lanes on the grid, which nothing else bounds: one large block
// among many small ones passes 2^32 lanes.  grid_slices cuts the blocks, in order, into runs [b0, b1) of at most max_run blocks
// with (largest rows in the run) x (blocks in the run) <= the limit, each with its own launches; a block above the limit is a
// run by itself (its tiles chain by ticket and look-back: a block cannot be split).  rows(b): what the chain's widest kernel
// puts on x for block b.  SHAFA_LACK_OF_MEMORY, before any device work, for a block whose rows x 256 lanes reach 2^32.
constexpr u64 RLE_GRID_ROWS = 1ull << 22;
constexpr u64 RLE_GRID_ROWS_MAX = (1ull << 24) - 1;
extern u64 g_rle_grid_rows;                        // api.hip, "rle_grid_rows": 0 = RLE_GRID_ROWS, else the limit (tests)
struct GridRun {
    int b0, b1;
    u32 rows;                                      // the largest of the run
};
template <typename Rows> inline int grid_slices(int nblocks, int max_run, Rows rows, std::vector<GridRun> &runs)
{
    const u64 limit = g_rle_grid_rows ? g_rle_grid_rows : RLE_GRID_ROWS;
    for (int b = 0; b < nblocks; ++b) {
        const u64 r = rows(b);
        if (r > RLE_GRID_ROWS_MAX) return SHAFA_LACK_OF_MEMORY;
        if (!runs.empty()) {
            GridRun &g = runs.back();
            const u64 top = r > g.rows ? r : g.rows;
            if (b - g.b0 < max_run && top * (u64)(b - g.b0 + 1) <= limit) {
                g.b1 = b + 1;
                g.rows = (u32)top;
                continue;
            }
        }
        runs.push_back(GridRun{b, b + 1, (u32)r});
    }
    return SHAFA_SUCCESS;
}

// ---- per-op parameter records (device arrays) --------------------------------------------------
struct EncBlk {
    const u8 *in;
    u8 *out;
    u64 n;
    u64 out_cap;
    u64 *out_n;
    int *err;
    const void *lut;
    u32 desc_base;
    u32 n_tiles;
    u32 ticket;
    u32 pad;
    const void *thist;     // sfe6 (sf_encode6.hip): the block's tile histograms (256 x u16 per 32 KiB tile), else unused
};

// second chain (descriptors, tickets) and per-block flags of the one-pass encoder's encode-again fall-back (sf_encode4.hip)
struct SfeRedo {
    u64 *desc2;
    u32 *tickets2;
    u32 *redo;
};

// ---- Module C planning rules, shared by sfenc_launch (sf_encode.hip) and sfenc_launch_dev (sf_encode_dev.hip) --------
// the code of symbol s (<= 32 bits: classes 1 and 2), len = t.len[s], right-aligned: its first four bytes, MSB first, shifted
// down.  (Bit by bit this was most of the 1.3 ms the host needed to prepare a 128-block launch.)
__host__ __device__ inline u32 sfe_code_value(const shafa_code_table &t, u32 s, u32 len)
{
    if (!len) return 0;
    const u8 *b = t.bits[s];
    const u32 be = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
    return len >= 32 ? be : be >> (32 - len);
}
// the look-up table entries of the three formats the encoder kernels read, from a symbol's code value and length
__host__ __device__ inline u32 sfe_entry32(u32 code, u32 len)           // code | len << 16; bit 31: no code
{
    return len ? (code | (len << 16)) : 0x80000000u;
}
__host__ __device__ inline u64 sfe_entry_pair(u32 code, u32 len)        // {code, len}; a symbol without a code: len = 1 << 16
{
    return len ? ((u64)code | ((u64)len << 32)) : (1ull << 48);
}
__host__ __device__ inline u64 sfe_entry64(u32 code, u32 len)           // code | len << 32
{
    return (u64)code | ((u64)len << 32);
}
// symbol s's entry in one of those formats, for the host's staging loop: the code value only where there is a code
// (computed first and selected after, the loop over a 128-block launch took twice as long)
template <typename Entry> inline auto sfe_entry(Entry entry, const shafa_code_table &t, u32 s)
{
    const u32 len = t.len[s];
    return len ? entry(sfe_code_value(t, s, len), len) : entry(0u, 0u);
}
// one-pass (chained) encoder or count / scan / pack for `count` blocks of class 1 (codes of <= 16 bits) or 2 (17..32 bits)
bool sfenc_one_pass(int cls, int count);

// ---- launchers (one per reference function) ------------------------------------------------------
// Module T on the device (sf_tables.hip): nblocks x 256 counts -> nblocks tables, both in device memory
int sftab_launch(Batch *bt, hipStream_t st, int nblocks, const u64 *d_freq, shafa_code_table *d_tables);
int hist_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                const u64 *h_in_n, u64 *d_freq);
// d_thist / h_thist_off (both or neither): also write every 32 KiB tile's own histogram (256 x u16) to d_thist + h_thist_off[b]
int hist_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                    const u64 *h_in_n, const u64 *d_n, u64 *d_freq, u8 *d_thist = nullptr, const u64 *h_thist_off = nullptr);
// d_thist / h_thist_off (both or neither): the tile histograms of shafa_hipd_hist256_tiles, block b's at d_thist + h_thist_off[b]
int sfenc_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                 const u64 *h_in_n, const shafa_code_table *h_tables, u8 *d_out, const u64 *h_out_off,
                 const u64 *h_out_cap, u64 *d_out_n, const u8 *d_thist = nullptr, const u64 *h_thist_off = nullptr);
// sfenc_launch with the block sizes and the tables in DEVICE memory (sf_encode_dev.hip): block b encodes d_in_n[b] <= h_in_cap[b]
// bytes with d_tables[b]; neither is read on the host
int sfenc_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, const shafa_code_table *d_tables, u8 *d_out, const u64 *h_out_off,
                     const u64 *h_out_cap, u64 *d_out_n, const u8 *d_thist, const u64 *h_thist_off);
int sfdec_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                 const u64 *h_in_n, const shafa_code_table *h_tables, const u64 *h_n_symbols, u8 *d_out,
                 const u64 *h_out_off);
int rleenc_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                  const u64 *h_in_n, u8 *d_out, const u64 *h_out_off, const u64 *h_out_cap, u64 *d_out_n,
                  u64 *d_freq, u8 *d_thist = nullptr, const u64 *h_thist_off = nullptr);
// sfdec_launch with the block sizes, symbol counts and tables in DEVICE memory (sfd_dev.hpp): none of them is read on the host
int sfdec_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, const shafa_code_table *d_tables, const u64 *d_n_symbols, u8 *d_out,
                     const u64 *h_out_off, const u64 *h_out_cap);
// Module C's kernel families behind sfenc_launch / sfenc_launch_dev: count / scan / pack (sf_encode3.hip), the one-pass chained
// encoder for codes of <= 16 and of 17..32 bits (sf_encode4.hip), the tile-histogram one-shot (sf_encode6.hip) and the generic
// form for device-planned lists (sf_encode.hip)
void sfenc3_launch(hipStream_t st, const EncBlk *dblk, int count, u32 max_tiles, u32 *d_tile_bits, u64 *d_tile_off, bool lut64);
int sfenc4_launch(hipStream_t st, const EncBlk *dblk, int count, u64 *d_desc, u32 *d_tickets, u32 lmax, u32 ragged, const SfeRedo &x);
int sfenc4_launch_long(hipStream_t st, const EncBlk *dblk, int count, u64 *d_desc, u32 *d_tickets, u32 lmax, u32 ragged, const SfeRedo &x);
bool sfenc4_needs_redo(u32 lmax);
bool sfenc4_long_ok();
int sfenc6_launch(hipStream_t st, const EncBlk *dblk, int count, u32 max_tiles, u32 lmax, bool any_ragged, u32 *d_tbits, u64 *d_toff);
void sfenc_generic_launch_dev(hipStream_t st, const EncBlk *dblk, u32 grid, u64 *d_desc, u32 *d_tickets, const u32 *d_plan);
extern int g_sfe_lanes;     // sf_encode4.hip: 0, or the workgroup width the one-pass encoder is held to (256 / 512)
// rledec_launch with the block sizes in DEVICE memory (descriptors laid out from h_in_cap)
int rledec_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                      const u64 *d_in_n, u8 *d_out, const u64 *h_out_off, const u64 *h_out_cap, u64 *d_out_n);
int rledec_launch(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off,
                  const u64 *h_in_n, u8 *d_out, const u64 *h_out_off, const u64 *h_out_cap, u64 *d_out_n);
// the sizes rledec_launch_dev would leave with h_out_cap = SHAFA_RLE_DECODE_MAX, without an output (rle_measure.hip)
int rlemeasure_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                          const u64 *d_in_n, u64 *d_out_n);
// the sizes rleenc_launch would leave for these input blocks with room enough, without an output (rle_encode_measure.hip)
int rleesize_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                        const u64 *d_in_n, u64 *d_out_n);
// the histograms and sizes rleenc_launch would leave for these input blocks with room enough, without an output
// (rle_encode_hist.hip); d_freq is overwritten
int rleehist_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                        const u64 *d_in_n, u64 *d_out_n, u64 *d_freq);
// where block b of a decoder's output (d_a_n[b] <= h_a_cap[b] bytes at d_a + h_a_off[b]) first differs from the h_ref_n[b] bytes
// at d_ref + h_ref_off[b], any alignment (compare.hip); the capacities' 8 KiB tiles number fewer than 2^31
int compare_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_a, const u64 *h_a_off, const u64 *h_a_cap,
                       const u64 *d_a_n, const u8 *d_ref, const u64 *h_ref_off, const u64 *h_ref_n, u64 *d_first);
// d_crc[b] = the CRC-32 of block b's d_in_n[b] <= h_in_cap[b] bytes at d_in + h_in_off[b], any alignment (crc32.hip); the
// capacities' 8 KiB tiles number fewer than 2^31
int crc32_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, u32 *d_crc);
// file f = blocks h_first[f] .. + h_count[f] of d_crc / d_n: the CRC-32 and the length of their concatenation (crc32.hip)
int crc32_combine_launch_dev(Batch *bt, hipStream_t st, int nfiles, const int *h_first, const int *h_count, const u32 *d_crc,
                             const u64 *d_n, u32 *d_file_crc, u64 *d_file_n);
// the positions of the pat_n pattern bytes in the blocks' regions (d_in_n[b] <= h_in_cap[b] bytes at d_in + h_in_off[b], any
// alignment), chained by h_flags (NULL = none), appended to d_hits from *d_total on (find.hip); the arguments have been checked
int find_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                    const u64 *d_in_n, const u8 *h_flags, const u64 *h_pos, const u8 *h_pat, u32 pat_n, u64 max_hits, u64 *d_hits,
                    u64 *d_count, u64 *d_total);
// block b's d_n[b] <= h_cap[b] elements of `elem` bytes at d_el + h_off[b] (any alignment) <-> their byte planes, plane j at
// d_planes + h_plane_off[b * elem + j] (multiples of 16): split reads d_el, merge writes it (planes.hip); the arguments have been
// checked and the capacities' tiles of SHAFA_PLANES_TILE elements number fewer than 2^31.  h_base_off non-NULL: every element is
// XORed with the element of the block's base region at d_base + h_base_off[b] (any alignment; SHAFA_PLANES_NO_BASE: none)
int planes_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off, const u64 *h_cap,
                      const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, const u8 *d_base, const u64 *h_base_off);
// the same transposes of the zigzag-folded differences to the element in front, every block starting afresh (planes.hip): split
// is one launch, merge three (tile sums, the blocks' scans, the merge) with 8 bytes of workspace more per tile of the capacities
int planes_diff_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                           const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off);
// the same with block b's differences taken to the element h_lag[b] >= 1 in front, the element side at multiples of elem
// (planes_lag.hip): split is one launch, merge up to three (column sums of the chunks, their scans, the merge) with elem bytes of
// workspace more per 8 elements of the capacities' tiles where a block has more than one chunk
int planes_lag_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                          const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, const u64 *h_lag);
// the same with block b's differences taken along up to SHAFA_PLANES_GRID_LAGS lags at once, h_lags[b * nlags + k] (the first
// >= 1, the others 0 or increasing: checked by the caller) (planes_lag.hip): split is one launch; merge is a first pass from the
// planes at the block's smallest lag — the merge of differences where that is 1 (planes_diff_merge_enqueue, planes.hip, on the
// caller's set-up, leaving the blocks with d_skip[b] != 0 alone), else the lag merge — and one pass in place per further lag
// fq (the _grid_quant entries, elem 4 or 8; checked by the caller): the elements are floats or doubles and the planes
// those of their codes.  split: the quantising split in the grid split's place, d_outl_n zeroed in front of it; merge: the chain
// as it is, then the restore in place and, where the call has a record, the patch
struct FieldQuant {
    const double *h_step, *h_bound;    // per block; the bound is the split's alone
    u64 *d_outl;                       // records of {position, bits}
    const u64 *h_outl_off;             // block b's first record
    const u64 *h_outl_count;           // split: its capacity in records; merge: its records
    u64 *d_outl_n;                     // split: the outliers found per block
    // the _grid_round entries (elem 2, 4 or 8): the quantiser is the rounding of the mantissa to h_keep[b] of its
    // h_mant[b] bits, h_step and h_bound are not looked at, and the kernels are the rounding ones
    bool round = false;
    const u32 *h_mant = nullptr, *h_keep = nullptr;
};
int planes_grid_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, bool merge, u8 *d_el, const u64 *h_off,
                           const u64 *h_cap, const u64 *d_n, u8 *d_planes, const u64 *h_plane_off, u32 nlags, const u64 *h_lags,
                           const FieldQuant *fq = nullptr);
// T(1 / step) as a double: the double division, rounded once to float at elem 4
double field_inverse(u32 elem, double step);
void planes_diff_merge_enqueue(u32 elem, const TileSetup &a, hipStream_t st, u8 *d_el, int nblocks, const u64 *d_n,
                               const u8 *d_planes, int *err, const u64 *d_skip);
// the histograms of the planes the grid split would write for these blocks, which may overlap, without the planes: d_freq[(b *
// elem + j) * 256 + s] counts byte s in plane j of block b (planes_lag.hip).  A row of h_lags that is all zeros: plain planes, no
// difference and no fold.  d_freq is zeroed first; the rows have been checked by the caller.
// fq: the same for the planes the quantising grid split would write (elem 4 or 8; rows, steps and bounds checked by the caller;
// DESIGN 7.31) or, fq->round, the rounding one (elem 2, 4 or 8; rows, h_mant and h_keep checked by the caller), and
// fq->d_outl_n[b] = the elements of block b that split would record, counted and not recorded; both are zeroed first.  The
// records' fields of fq are not looked at
int planes_grid_hist_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, const u8 *d_el, const u64 *h_off, const u64 *h_cap,
                                const u64 *d_n, u32 nlags, const u64 *h_lags, const FieldQuant *fq, u64 *d_freq);
// the error statistics of the blocks at d_el + h_off[b] (elem 2, 4 or 8; everything checked by the caller), one record of
// SHAFA_ERR_WORDS words a block at d_stat.  ERR_PAIR (shafa_hipd_error_dev): d_el is what came back, at multiples of
// 16, the originals lie at d_ref + h_ref_off[b], and h_mant, h_abs and h_rel are the blocks'.  ERR_QUANT (elem 4 or 8) and
// ERR_ROUND: d_el is the original and what comes back is made from it under h_step and h_bound, or h_mant and h_keep.
enum ErrSrc { ERR_PAIR = 0, ERR_QUANT = 1, ERR_ROUND = 2 };
struct ErrorArgs {
    ErrSrc src;
    const u32 *h_mant, *h_keep;
    const double *h_step, *h_bound, *h_abs, *h_rel;
    const u8 *d_ref;
    const u64 *h_ref_off;
};
int planes_error_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 elem, const ErrorArgs &e, const u8 *d_el, const u64 *h_off,
                            const u64 *h_cap, const u64 *d_n, u64 *d_stat);
// block b's d_n[b] <= h_cap[b] records of `width` = 1 .. SHAFA_RECORDS_MAX_WIDTH bytes at d_rec + h_off[b] (any alignment) <-> their
// byte columns, column j at d_planes + h_plane_off[b * width + j] (multiples of 16): split reads d_rec, merge writes it
// (records.hip); the arguments have been checked and the capacities' tiles of SHAFA_RECORDS_TILE records number fewer than 2^31
int records_launch_dev(Batch *bt, hipStream_t st, int nblocks, u32 width, bool merge, u8 *d_rec, const u64 *h_off, const u64 *h_cap,
                       const u64 *d_n, u8 *d_planes, const u64 *h_plane_off);
// the checkpoints of blocks of SF-decoded bytes, every `span` symbols (seek.hip); the capacities' spans number fewer than 2^31
int seek_index_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                          const u64 *d_in_n, const shafa_code_table *d_tables, u32 span, int flags, const u64 *h_ckpt_first,
                          u64 *d_ckpt, u32 *d_status, u64 *d_out_n);
// the bytes [lo, hi) of the items' blocks, decoded from the checkpoints that cover them (seek.hip); every item has been checked
// against its block
int read_spans_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_file, const u64 *h_pay_off, const u64 *h_pay_n,
                          const u64 *h_n_symbols, const u64 *h_ckpt_first, const shafa_code_table *d_tables, u32 span, int flags,
                          const u64 *d_ckpt, int nitems, const int *h_item_block, const u64 *h_item_first,
                          const u64 *h_item_last, const u64 *h_item_lo, const u64 *h_item_hi, const u64 *h_item_dst, u8 *d_out);
// the sizes sfenc_launch_dev would leave for blocks with these histograms and tables and room enough (sf_encoded_size.hip)
int sfesize_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u64 *d_freq, const shafa_code_table *d_tables, u64 *d_out_n);
// pack.hip's payload movers (pack_bulk, pack_seams) on records laid out elsewhere (unpack.hip): block b moves n bytes from src
// to dst, no header.  pack_bulk writes the 16-byte destination words inside [dst, dst + n) and needs src 16-aligned whenever
// (src - dst) is not a multiple of 16 — read the record of d_bulk; pack_seams writes every other byte — from d_seam.  Both
// return at once when *d_verdict is 0.  max_n bounds every record's n + 15 (the bulk grid).
struct MoveDesc {
    const u8 *src;
    u8 *dst;
    u64 n;
    u64 hdr_val;    // 0
    u32 hdr_len;    // 0
    u32 pad;
};
int pack_move_launch(hipStream_t st, int nblocks, const MoveDesc *d_bulk, const MoveDesc *d_seam, const u32 *d_verdict,
                     u64 max_n);
void sfenc_configure(int sfe4_min_blocks);
void sfdec_configure(int speculate);
void sfdec_configure_path(int path);
void rleenc_configure(int force_general);
int gen_launch(hipStream_t st, u64 seed, u64 first, const u8 *d_map, u8 *d_out, size_t n);

// ---- api.hip, for layer 3 (pipe.hip) ----------------------------------------------------------------
int api_lazy_init();                          // shafa_hip_init(0) unless a device was selected already
int api_pipe_device(int slot, int n_slots);   // device of slot `slot` of a pipe of n_slots (shafa_hip_init_devices), else the layer-1 device
