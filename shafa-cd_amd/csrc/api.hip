// api.hip — the C-ABI of libshafa_hip.so (include/shafa_hip.h): lifecycle, batch contexts and the
// host-buffer one-block wrappers that stand where the reference calls block_compression / make_freq
// (f.c:248,310,325), compress_to_buffer (c.c:411) and the decompressors (d.c:342,735).
#include "common.hpp"
#include "internal.hpp"

#include <cmath>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>

// ------------------------------------------------------------------------------------------------
// error text (per calling thread: the reference's drivers call the per-block functions from one thread per block)
// ------------------------------------------------------------------------------------------------
static thread_local char g_last_error[512] = "";
u64 g_rle_grid_rows = 0;                     // "rle_grid_rows" (internal.hpp, grid_slices)

int shafa_set_hip_error(hipError_t e, const char *what)
{
    snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, hipGetErrorString(e));
    return SHAFA_DEVICE_ERROR;
}

// ------------------------------------------------------------------------------------------------
// batch context
// ------------------------------------------------------------------------------------------------
int batch_enter(Batch *b, hipStream_t st)
{
    if (!b) return SHAFA_OUTSIDE_MODULE;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != b->device) {
        snprintf(g_last_error, sizeof(g_last_error), "batch of device %d used while device %d is current", b->device, dev);
        return SHAFA_DEVICE_ERROR;
    }
    if (b->has_last && b->last_st != st) {
        const hipError_t e = hipStreamSynchronize(b->last_st);
        if (e == hipErrorInvalidHandle || e == hipErrorInvalidResourceHandle || e == hipErrorContextIsDestroyed)
            (void)hipGetLastError();       // the previous stream was destroyed by its owner (legal once its work is done): nothing to wait for
        else if (e != hipSuccess)          // a kernel or copy on it failed: the workspace and the error words cannot be trusted
            return shafa_set_hip_error(e, "hipStreamSynchronize(previous stream of the batch)");
    }
    b->last_st = st;
    b->has_last = true;
    return SHAFA_SUCCESS;
}

int batch_reserve(Batch *b, hipStream_t st, size_t bytes)
{
    if (bytes <= b->ws_bytes) return SHAFA_SUCCESS;
    if (b->d_ws) {
        HIP_TRY(hipStreamSynchronize(st));          // kernels of earlier launches on this batch's stream
        HIP_TRY(hipFree(b->d_ws));
        b->d_ws = nullptr;
        b->ws_bytes = 0;
    }
    const size_t want = bytes + bytes / 8 + 4096;
    HIP_TRY(hipMalloc(&b->d_ws, want));
    b->ws_bytes = want;
    return SHAFA_SUCCESS;
}

static void seg_release(StageSeg &s, bool wait)
{
    if (s.ev) {
        if (wait && s.sealed) (void)hipEventSynchronize(s.ev);
        (void)hipEventDestroy(s.ev);
        s.ev = nullptr;
    }
}

void *batch_stage(Batch *b, hipStream_t st, size_t bytes)
{
    bytes = (bytes + 63) & ~(size_t)63;
    if (!b->segs) b->segs = new std::vector<StageSeg>();
    std::vector<StageSeg> &segs = *b->segs;
    // seal the previous region: its copies were enqueued by the caller after it was handed out
    if (!segs.empty() && !segs.back().sealed) {
        if (hipEventRecord(segs.back().ev, segs.back().st) != hipSuccess) return nullptr;
        segs.back().sealed = true;
    }
    if (bytes > b->stage_bytes) {          // grow: wait for the copies that still read the old arena (their events only)
        for (StageSeg &s : segs) seg_release(s, true);
        segs.clear();
        if (b->h_stage) (void)hipHostFree(b->h_stage);
        b->h_stage = nullptr;
        b->stage_bytes = 0;
        const size_t want = 4 * bytes + (1 << 20);
        if (hipHostMalloc((void **)&b->h_stage, want, hipHostMallocDefault) != hipSuccess) return nullptr;
        b->stage_bytes = want;
        b->stage_used = 0;
    }
    size_t off = b->stage_used;
    if (off + bytes > b->stage_bytes) off = 0;                 // wrap
    // regions that overlap the new one must have been consumed: wait for exactly their events
    for (size_t i = 0; i < segs.size();) {
        StageSeg &s = segs[i];
        if (s.off < off + bytes && off < s.off + s.bytes) {
            seg_release(s, true);
            segs.erase(segs.begin() + (long)i);
        } else ++i;
    }
    StageSeg seg = {off, bytes, st, nullptr, false};
    if (hipEventCreateWithFlags(&seg.ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    segs.push_back(seg);
    b->stage_used = off + bytes;
    return b->h_stage + off;
}

u8 *batch_params_begin(Batch *b, size_t bytes)
{
    if (!b->copy_st) {
        if (hipStreamCreateWithFlags(&b->copy_st, hipStreamNonBlocking) != hipSuccess) return nullptr;
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&b->par_ready[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&b->par_free[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    const int i = b->par_turn;
    b->par_turn ^= 1;
    b->par_cur = i;
    b->par_inline = !b->par_dma && bytes <= PARAMS_INLINE_BYTES;   // the caller stages on the stream that will read the staging arena
    if (bytes > b->par_bytes[i]) {                     // grow: the kernels that read the old buffer must be through
        if (b->par_used[i] && hipEventSynchronize(b->par_free[i]) != hipSuccess) return nullptr;
        if (b->d_par[i]) (void)hipFree(b->d_par[i]);
        b->d_par[i] = nullptr;
        b->par_bytes[i] = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipMalloc(&b->d_par[i], want) != hipSuccess) return nullptr;
        b->par_bytes[i] = want;
    }
    return (u8 *)b->d_par[i];
}

// The parameter upload as a kernel that reads the pinned staging arena (host memory the device can address): above 16 KB
// hipMemcpyAsync hands a host-to-device copy to the SDMA engine, and a launch of 8..30 blocks then waited ~0.6 ms for its
// 17..60 KB of parameters (tools/dbg/small_launch_encode.sh: 8 x 64 MiB encoded in 790 us, 7 x 64 MiB in 190 us).
// Except in a pipe (layer 3): there the link is busy with the blocks themselves and a kernel's reads of host memory queue
// behind 64 MiB transfers (decode 41 -> 34 GiB/s, tools/dbg/pipe_rate_ab.sh), while the engine's latency hides behind the
// block's own transfer as long as the copy is NOT in the slot's stream (there it starts after the block has arrived: 33
// GiB/s as well): a pipe slot's batch (par_dma) keeps hipMemcpyAsync on the side stream.
__global__ __launch_bounds__(256) void param_copy_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// The small per-launch records of the other launchers (hist, rle_encode, rle_decode), in the launch's stream: the same
// kernel once the runtime would take the SDMA engine for them (more than 16 KB: hundreds of blocks), hipMemcpyAsync below
// that and in a pipe.  `src` is in the batch's pinned staging arena (64-byte units), `dst` 16-byte aligned with room for
// the last piece.
int batch_upload(Batch *b, hipStream_t st, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return SHAFA_SUCCESS;
    if (b->par_dma || bytes <= 16384 || (bytes & 15) || ((uintptr_t)dst & 15)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return SHAFA_SUCCESS;
    }
    const size_t n16 = bytes / 16, wgs = (n16 + 255) / 256;
    hipLaunchKernelGGL(param_copy_kernel, dim3((unsigned)(wgs < 512 ? wgs : 512)), dim3(256), 0, st, (uint4 *)dst, (const uint4 *)src, n16);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}

int batch_params_commit(Batch *b, hipStream_t st, const void *hs, size_t bytes)
{
    const int i = b->par_cur;
    const size_t n16 = (bytes + 15) / 16;              // the arena is handed out in 64-byte units, the device buffer has slack
    const size_t wgs = (n16 + 255) / 256;
    if (b->par_inline) {
        // a few blocks' worth (layer 3 submits one block per launch): in the launch's own stream, in order — a pipe's slots
        // already outnumber the hardware queues, and a side stream's kernel would wait behind another slot's kernels
        if (n16) {
            hipLaunchKernelGGL(param_copy_kernel, dim3((unsigned)wgs), dim3(256), 0, st, (uint4 *)b->d_par[i], (const uint4 *)hs, n16);
            HIP_TRY(hipGetLastError());
        }
        return SHAFA_SUCCESS;
    }
    if (b->par_used[i]) HIP_TRY(hipStreamWaitEvent(b->copy_st, b->par_free[i], 0));
    if (b->par_dma) {
        if (bytes) HIP_TRY(hipMemcpyAsync(b->d_par[i], hs, bytes, hipMemcpyHostToDevice, b->copy_st));
    } else if (n16) {
        hipLaunchKernelGGL(param_copy_kernel, dim3((unsigned)(wgs < 512 ? wgs : 512)), dim3(256), 0, b->copy_st,
                           (uint4 *)b->d_par[i], (const uint4 *)hs, n16);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(b->par_ready[i], b->copy_st));
    HIP_TRY(hipStreamWaitEvent(st, b->par_ready[i], 0));
    return SHAFA_SUCCESS;
}

int batch_params_done(Batch *b, hipStream_t st)
{
    HIP_TRY(hipEventRecord(b->par_free[b->par_cur], st));
    b->par_used[b->par_cur] = true;
    return SHAFA_SUCCESS;
}

void batch_stage_retire(Batch *b, hipStream_t st)
{
    if (!b->segs) return;
    std::vector<StageSeg> &segs = *b->segs;
    for (size_t i = 0; i < segs.size();) {
        if (segs[i].st == st) {
            seg_release(segs[i], false);
            segs.erase(segs.begin() + (long)i);
        } else ++i;
    }
    if (segs.empty()) b->stage_used = 0;
}

int tile_count(int nblocks, const u64 *h_cap, u64 unit, u64 *ntiles)
{
    u64 n = 0;
    for (int b = 0; b < nblocks; ++b)
        if ((n += h_cap[b] / unit + (h_cap[b] % unit != 0)) > 0x7FFFFFFFull) return b;
    if (ntiles) *ntiles = n;
    return nblocks;
}

// such a part: h's bytes (NULL: zeros), zero padded to the next part
static void put16(u8 *dst, const void *h, size_t bytes)
{
    if (h) memcpy(dst, h, bytes);
    else memset(dst, 0, bytes);
    memset(dst + bytes, 0, (0 - bytes) & 15);
}

// the layout is described once, in internal.hpp
int tile_setup(Batch *bt, hipStream_t st, int nblocks, const u64 *h_off, const u64 *h_cap, u32 unit, const TileExtra *extras,
               int nextras, size_t scratch_per_tile, size_t scratch_fixed, TileSetup *s)
{
    u64 ntiles = 0;
    if (tile_count(nblocks, h_cap, unit, &ntiles) < nblocks) return SHAFA_LACK_OF_MEMORY;
    const size_t nb = (size_t)nblocks;
    size_t o_up = 0, up_bytes = 0, u_extra[TILE_EXTRAS] = {};
    take16(o_up, (size_t)ntiles * scratch_per_tile + scratch_fixed);
    const size_t u_off = take16(up_bytes, nb * 8), u_cap = take16(up_bytes, nb * 8);
    for (int i = 0; i < nextras; ++i) u_extra[i] = take16(up_bytes, extras[i].bytes);
    const size_t u_base = take16(up_bytes, (nb + 1) * 4);
    int rc = batch_reserve(bt, st, o_up + up_bytes);
    if (rc) return rc;
    u8 *up = (u8 *)bt->d_ws + o_up;
    u8 *hs = (u8 *)batch_stage(bt, st, up_bytes);
    if (!hs) return SHAFA_LACK_OF_MEMORY;
    put16(hs + u_off, h_off, nb * 8);
    put16(hs + u_cap, h_cap, nb * 8);
    for (int i = 0; i < nextras; ++i) put16(hs + u_extra[i], extras[i].h, extras[i].bytes);
    u32 *hb = (u32 *)(hs + u_base);
    u32 base = 0;
    for (int b = 0; b < nblocks; ++b) {
        hb[b] = base;
        base += (u32)(h_cap[b] / unit + (h_cap[b] % unit != 0));
    }
    hb[nblocks] = base;
    memset(hb + nb + 1, 0, (0 - (nb + 1) * 4) & 15);
    if ((rc = batch_upload(bt, st, up, hs, up_bytes))) return rc;
    s->off = (const u64 *)(up + u_off);
    s->cap = (const u64 *)(up + u_cap);
    for (int i = 0; i < TILE_EXTRAS; ++i) s->extra[i] = i < nextras ? up + u_extra[i] : nullptr;
    s->tbase = (const u32 *)(up + u_base);
    s->scratch = (u8 *)bt->d_ws;
    s->nt = (u32)ntiles;
    s->per_wg = s->nt ? (s->nt + TP_MAX_WGS - 1) / TP_MAX_WGS : 1;
    s->wgs = (s->nt + s->per_wg - 1) / s->per_wg;
    return SHAFA_SUCCESS;
}

// the argument checks of the size entries (shafa_hipd_rle_decoded_size_dev, shafa_hipd_rle_encoded_size_dev,
// shafa_hipd_rle_encoded_hist_dev), of shafa_hipd_compare_dev's side a and of shafa_hipd_crc32_dev (whose regions need no
// alignment: aligned = false), before HIP is touched: true = go on, false = the call returns *rc
static bool size_pass_check(Batch *b, int nblocks, const u64 *h_in_off, const u64 *h_in_cap, const u64 *d_in_n,
                            const void *d_out_n, int *rc, bool aligned = true)
{
    *rc = SHAFA_OUTSIDE_MODULE;
    if (!b || !d_in_n || !d_out_n) return false;
    *rc = SHAFA_SUCCESS;
    if (nblocks <= 0) return false;
    *rc = SHAFA_LACK_OF_MEMORY;
    if (nblocks > b->max_blocks) return false;
    *rc = SHAFA_OUTSIDE_MODULE;
    if (!h_in_off || !h_in_cap) return false;
    for (int i = 0; aligned && i < nblocks; ++i)
        if (h_in_off[i] & 15) return false;
    *rc = SHAFA_SUCCESS;
    return true;
}

// those checks, then the batch's: true = launch the pass
static bool size_pass_enter(Batch *b, hipStream_t st, int nblocks, const u64 *h_in_off, const u64 *h_in_cap, const u64 *d_in_n,
                            const u64 *d_out_n, int *rc)
{
    return size_pass_check(b, nblocks, h_in_off, h_in_cap, d_in_n, d_out_n, rc) && (*rc = batch_enter(b, st)) == SHAFA_SUCCESS;
}

static int size_pass_dev(int (*launch)(Batch *, hipStream_t, int, const u8 *, const u64 *, const u64 *, const u64 *, u64 *),
                         Batch *b, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                         const u64 *d_in_n, u64 *d_out_n)
{
    int rc;
    if (!size_pass_enter(b, st, nblocks, h_in_off, h_in_cap, d_in_n, d_out_n, &rc)) return rc;
    return launch(b, st, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_out_n);
}

extern "C" {

int shafa_hip_abi_version(void) { return SHAFA_HIP_ABI_VERSION; }

int shafa_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *shafa_hip_last_error(void) { return g_last_error; }

int shafa_hip_set_option(const char *name, long value)
{
    if (name && !strcmp(name, "sf_encode_one_pass_min_blocks")) {
        sfenc_configure(value < 0 ? 0 : (value > (1 << 30) ? (1 << 30) : (int)value));      // 0: measured defaults
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "sf_encode_window_bits")) {
        extern int g_sfe_window_bits;
        if (value < 0 || value > 16) return SHAFA_OUTSIDE_MODULE;
        g_sfe_window_bits = (int)value;
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "sf_encode_lanes")) {
        if (value != 0 && value != 256 && value != 512) return SHAFA_OUTSIDE_MODULE;
        g_sfe_lanes = (int)value;
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "sf_decode_path")) {
        if (value < 0 || value > 2) return SHAFA_OUTSIDE_MODULE;
        sfdec_configure_path((int)value);
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "rle_encode_general")) {
        rleenc_configure(value != 0);
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "rle_grid_rows")) {
        if (value < 0) return SHAFA_OUTSIDE_MODULE;
        g_rle_grid_rows = (u64)value < RLE_GRID_ROWS_MAX ? (u64)value : RLE_GRID_ROWS_MAX;      // 0: RLE_GRID_ROWS
        return SHAFA_SUCCESS;
    }
    if (name && !strcmp(name, "rle_encode_one_pass"))       // the one-pass form is gone: 0 (the two-pass kernels) is all there is
        return value == 0 ? SHAFA_SUCCESS : SHAFA_OUTSIDE_MODULE;
    if (name && !strcmp(name, "sf_decode_speculate")) {
        sfdec_configure(value <= 0 ? 0 : value >= 2 ? 2 : 1);
        return SHAFA_SUCCESS;
    }
    return SHAFA_OUTSIDE_MODULE;
}

int shafa_hipd_batch_create(int max_blocks, size_t max_block_bytes, shafa_hipd_batch **out)
{
    if (!out || max_blocks <= 0) return SHAFA_OUTSIDE_MODULE;
    Batch *b = (Batch *)calloc(1, sizeof(Batch));
    if (!b) return SHAFA_LACK_OF_MEMORY;
    b->max_blocks = max_blocks;
    b->max_block_bytes = max_block_bytes;
    if (hipGetDevice(&b->device) != hipSuccess) { free(b); return SHAFA_DEVICE_ERROR; }
    b->h_hosterr = (int *)calloc((size_t)max_blocks, sizeof(int));
    if (!b->h_hosterr) { free(b); return SHAFA_LACK_OF_MEMORY; }
    hipError_t e = hipMalloc((void **)&b->d_err, (size_t)max_blocks * sizeof(int));
    if (e == hipSuccess) e = hipMemset(b->d_err, 0, (size_t)max_blocks * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&b->d_par_hist, (size_t)max_blocks * 48);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_err, (size_t)max_blocks * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) {
        if (b->d_err) hipFree(b->d_err);
        free(b);
        return shafa_set_hip_error(e, "shafa_hipd_batch_create");
    }
    *out = (shafa_hipd_batch *)b;
    return SHAFA_SUCCESS;
}

void shafa_hipd_batch_destroy(shafa_hipd_batch *hb)
{
    Batch *b = (Batch *)hb;
    if (!b) return;
    DeviceGuard dg(b->device);                     // the batch's device, whatever the caller's current device is
    if (b->has_last) (void)hipStreamSynchronize(b->last_st);
    hipDeviceSynchronize();
    if (b->copy_st) {
        (void)hipStreamDestroy(b->copy_st);
        for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(b->par_ready[i]); (void)hipEventDestroy(b->par_free[i]); }
    }
    for (int i = 0; i < 2; ++i)
        if (b->d_par[i]) hipFree(b->d_par[i]);
    if (b->d_ws) hipFree(b->d_ws);
    if (b->segs) {
        for (StageSeg &sg : *b->segs) seg_release(sg, false);
        delete b->segs;
    }
    if (b->h_stage) hipHostFree(b->h_stage);
    if (b->d_err) hipFree(b->d_err);
    if (b->d_par_hist) hipFree(b->d_par_hist);
    if (b->h_err) hipHostFree(b->h_err);
    free(b->h_hosterr);
    free(b);
}

int shafa_hipd_hist256(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                       const uint64_t *h_in_off, const uint64_t *h_in_n, uint64_t *d_freq)
{
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return hist_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, d_freq);
}

int shafa_hipd_sf_build_codes(shafa_hipd_batch *b, void *stream, int nblocks, const uint64_t *d_freq, shafa_code_table *d_tables)
{
    if (!d_freq || !d_tables) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sftab_launch((Batch *)b, (hipStream_t)stream, nblocks, d_freq, d_tables);
}

size_t shafa_hip_tile_hist_bytes(size_t n) { return ((n + SHAFA_TILE_BYTES - 1) / SHAFA_TILE_BYTES) * 512; }

int shafa_hipd_hist256_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_n, uint64_t *d_freq,
                             uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off)
{
    if (!d_tile_hist || !h_tile_hist_off) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return hist_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, nullptr, d_freq, d_tile_hist,
                           h_tile_hist_off);
}

int shafa_hipd_rle_encode_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                                const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n,
                                uint64_t *d_freq, uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off)
{
    if (!d_freq || !d_tile_hist || !h_tile_hist_off) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return rleenc_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, d_out, h_out_off,
                         h_out_cap, d_out_n, d_freq, d_tile_hist, h_tile_hist_off);
}

int shafa_hipd_sf_encode_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_n, const shafa_code_table *h_tables,
                               const uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off, uint8_t *d_out,
                               const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n)
{
    if (!d_tile_hist || !h_tile_hist_off) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfenc_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, h_tables, d_out,
                        h_out_off, h_out_cap, d_out_n, d_tile_hist, h_tile_hist_off);
}

int shafa_hipd_sf_encode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                             const shafa_code_table *d_tables, const uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off,
                             uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n)
{
    if (!b || !d_in_n || !d_tables) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfenc_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_tables, d_out,
                            h_out_off, h_out_cap, d_out_n, d_tile_hist, h_tile_hist_off);
}

int shafa_hipd_rle_encode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                          const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                          const uint64_t *h_out_off, const uint64_t *h_out_cap,
                          uint64_t *d_out_n, uint64_t *d_freq)
{
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return rleenc_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, d_out, h_out_off,
                         h_out_cap, d_out_n, d_freq);
}

int shafa_hipd_sf_encode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                         const uint64_t *h_in_off, const uint64_t *h_in_n,
                         const shafa_code_table *h_tables, uint8_t *d_out, const uint64_t *h_out_off,
                         const uint64_t *h_out_cap, uint64_t *d_out_n)
{
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfenc_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, h_tables, d_out,
                        h_out_off, h_out_cap, d_out_n);
}

int shafa_hipd_sf_decode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                         const uint64_t *h_in_off, const uint64_t *h_in_n,
                         const shafa_code_table *h_tables, const uint64_t *h_n_symbols,
                         uint8_t *d_out, const uint64_t *h_out_off)
{
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfdec_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, h_tables,
                        h_n_symbols, d_out, h_out_off);
}

int shafa_hipd_rle_decode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                          const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                          const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n)
{
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return rledec_launch((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_n, d_out, h_out_off,
                         h_out_cap, d_out_n);
}

int shafa_hipd_sf_decode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                             const shafa_code_table *d_tables, const uint64_t *d_n_symbols,
                             uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap)
{
    if (!b || !d_in_n || !d_tables || !d_n_symbols) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfdec_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_tables,
                            d_n_symbols, d_out, h_out_off, h_out_cap);
}

int shafa_hipd_rle_decode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                              const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                              uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n)
{
    if (!b || !d_in_n) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return rledec_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_out, h_out_off,
                             h_out_cap, d_out_n);
}

int shafa_hipd_rle_decoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n)
{
    return size_pass_dev(rlemeasure_launch_dev, (Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n,
                         d_out_n);
}

int shafa_hipd_rle_encoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n)
{
    return size_pass_dev(rleesize_launch_dev, (Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n,
                         d_out_n);
}

int shafa_hipd_rle_encoded_hist_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n, uint64_t *d_freq)
{
    if (!b || !d_freq) return SHAFA_OUTSIDE_MODULE;
    int rc;
    if (!size_pass_enter((Batch *)b, (hipStream_t)stream, nblocks, h_in_off, h_in_cap, d_in_n, d_out_n, &rc)) return rc;
    return rleehist_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_out_n, d_freq);
}

int shafa_hipd_compare_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_a, const uint64_t *h_a_off,
                           const uint64_t *h_a_cap, const uint64_t *d_a_n, const uint8_t *d_ref, const uint64_t *h_ref_off,
                           const uint64_t *h_ref_n, uint64_t *d_first)
{
    if (!d_a || !d_ref || ((uintptr_t)d_a & 15)) return SHAFA_OUTSIDE_MODULE;
    int rc;
    if (!size_pass_check((Batch *)b, nblocks, h_a_off, h_a_cap, d_a_n, d_first, &rc)) return rc;
    if (!h_ref_off || !h_ref_n) return SHAFA_OUTSIDE_MODULE;
    if (tile_count(nblocks, h_a_cap, 8192) < nblocks) return SHAFA_LACK_OF_MEMORY;      // 8 KiB tiles of the capacities
    if ((rc = batch_enter((Batch *)b, (hipStream_t)stream))) return rc;
    return compare_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_a, h_a_off, h_a_cap, d_a_n, d_ref, h_ref_off, h_ref_n,
                              d_first);
}

int shafa_hipd_crc32_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                         const uint64_t *h_in_cap, const uint64_t *d_in_n, uint32_t *d_crc)
{
    if (!b || !d_in) return SHAFA_OUTSIDE_MODULE;
    int rc;
    if (!size_pass_check((Batch *)b, nblocks, h_in_off, h_in_cap, d_in_n, d_crc, &rc, false)) return rc;
    if (tile_count(nblocks, h_in_cap, 8192) < nblocks) return SHAFA_LACK_OF_MEMORY;     // 8 KiB tiles of the capacities
    if ((rc = batch_enter((Batch *)b, (hipStream_t)stream))) return rc;
    return crc32_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, d_crc);
}

int shafa_hipd_crc32_combine_dev(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                                 const uint32_t *d_crc, const uint64_t *d_n, uint32_t *d_file_crc, uint64_t *d_file_n)
{
    if (!b || !d_crc || !d_n || !d_file_crc || !d_file_n) return SHAFA_OUTSIDE_MODULE;
    if (nfiles <= 0) return SHAFA_SUCCESS;
    if (nfiles > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_first || !h_count) return SHAFA_OUTSIDE_MODULE;
    for (int f = 0; f < nfiles; ++f)
        if (h_first[f] < 0 || h_count[f] < 0 || h_count[f] > 0x7FFFFFFF - h_first[f]) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return crc32_combine_launch_dev((Batch *)b, (hipStream_t)stream, nfiles, h_first, h_count, d_crc, d_n, d_file_crc, d_file_n);
}

int shafa_hipd_find_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                        const uint64_t *h_in_cap, const uint64_t *d_in_n, const uint8_t *h_flags, const uint64_t *h_pos,
                        const uint8_t *h_pat, uint32_t pat_n, uint64_t max_hits, uint64_t *d_hits, uint64_t *d_count,
                        uint64_t *d_total)
{
    if (!b || !d_in || !d_in_n || !d_count || !d_total || !h_pat) return SHAFA_OUTSIDE_MODULE;
    if (pat_n == 0 || pat_n > SHAFA_FIND_MAX_PATTERN || (max_hits && !d_hits)) return SHAFA_OUTSIDE_MODULE;
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_in_cap) return SHAFA_OUTSIDE_MODULE;
    if (tile_count(nblocks, h_in_cap, 8192) < nblocks) return SHAFA_LACK_OF_MEMORY;     // 8 KiB tiles of the capacities
    if (!h_in_off || !h_pos) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; h_flags && i < nblocks; ++i)
        if (h_flags[i] & ~(SHAFA_FIND_NEXT | SHAFA_FIND_CONTEXT)) return SHAFA_OUTSIDE_MODULE;
    if (h_flags && (h_flags[nblocks - 1] & SHAFA_FIND_NEXT)) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return find_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n, h_flags, h_pos, h_pat,
                           pat_n, max_hits, d_hits, d_count, d_total);
}

// the checks the plane and the record transposes share (include/shafa_hip.h), in one order, then the launch.  d_el is the element
// or record side; `unit` the bytes of an element (1, 2, 4 or 8) or, TR_RECORDS, of a record (1 .. SHAFA_RECORDS_MAX_WIDTH);
// TR_XOR: the _xor entries, with a base side; TR_DIFF: the _diff entries; TR_LAG: the _lag entries, with a lag a block (h_lag) and
// the element side at multiples of the element; TR_GRID: the _grid entries, the same with nlags (1 .. SHAFA_PLANES_GRID_LAGS)
// lags a block in h_lag
enum Transpose { TR_PLANES, TR_XOR, TR_DIFF, TR_LAG, TR_GRID, TR_RECORDS };
static_assert(SHAFA_RECORDS_TILE == SHAFA_PLANES_TILE, "one tile for the plane and the record entries");

// a step or a bound of the _grid_quant entries: finite, normal, > 0 and exactly a T (float at elem 4); a step's inverse as T is
// finite and not 0 as well
static bool field_param_ok(uint32_t elem, double v, bool step)
{
    if (!std::isnormal(v) || v <= 0) return false;
    if (elem == 4 && (!std::isnormal((float)v) || (double)(float)v != v)) return false;
    if (!step) return true;
    const double inv = field_inverse(elem, v);
    return std::isfinite(inv) && inv != 0;
}

// the steps of a call's blocks and, where the entry takes them (h_bound non-NULL), the bounds
static bool field_params_ok(uint32_t elem, int nblocks, const double *h_step, const double *h_bound)
{
    for (int i = 0; i < nblocks; ++i)
        if (!field_param_ok(elem, h_step[i], true) || (h_bound && !field_param_ok(elem, h_bound[i], false))) return false;
    return true;
}

// the mantissa widths and the kept bits of the _grid_round entries' blocks: the format's mant for elem — 7 (bfloat16)
// or 10 (float16) at 2, 23 at 4, 52 at 8 — and keep <= mant
static bool round_params_ok(uint32_t elem, int nblocks, const uint32_t *h_mant, const uint32_t *h_keep)
{
    for (int i = 0; i < nblocks; ++i) {
        const uint32_t m = h_mant[i];
        if (elem == 2 ? m != 7 && m != 10 : m != (elem == 4 ? 23u : 52u)) return false;
        if (h_keep[i] > m) return false;
    }
    return true;
}

static int transpose_dev(bool merge, Transpose tr, shafa_hipd_batch *b, void *stream, int nblocks, uint32_t unit, const uint8_t *d_el,
                         const uint64_t *h_off, const uint8_t *d_base, const uint64_t *h_base_off, const uint64_t *h_cap,
                         const uint64_t *d_n, const uint8_t *d_planes, const uint64_t *h_plane_off, const uint64_t *h_lag = nullptr,
                         uint32_t nlags = 1, const FieldQuant *fq = nullptr)
{
    const bool xr = tr == TR_XOR;
    if (!b || !d_el || !d_planes || !d_n || (xr && !d_base)) return SHAFA_OUTSIDE_MODULE;
    if (tr == TR_GRID && (nlags < 1 || nlags > SHAFA_PLANES_GRID_LAGS)) return SHAFA_OUTSIDE_MODULE;
    if (tr == TR_RECORDS ? unit < 1 || unit > SHAFA_RECORDS_MAX_WIDTH : unit != 1 && unit != 2 && unit != 4 && unit != 8)
        return SHAFA_OUTSIDE_MODULE;
    if (fq && unit != 4 && unit != 8 && !(fq->round && unit == 2)) return SHAFA_OUTSIDE_MODULE;    // floats and doubles; rounding: 16 bits too
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_cap) return SHAFA_OUTSIDE_MODULE;
    u64 bytes = 0;
    for (int i = 0; i < nblocks; ++i) {
        if (h_cap[i] > ~0ull / unit || bytes + h_cap[i] * unit < bytes) return SHAFA_LACK_OF_MEMORY;
        bytes += h_cap[i] * unit;
    }
    if (tile_count(nblocks, h_cap, SHAFA_PLANES_TILE) < nblocks) return SHAFA_LACK_OF_MEMORY;    // tiles of elements or records
    if (!h_off || !h_plane_off || (xr && !h_base_off) || ((uintptr_t)d_planes & 15)) return SHAFA_OUTSIDE_MODULE;
    for (size_t i = 0; i < (size_t)nblocks * unit; ++i)
        if (h_plane_off[i] & 15) return SHAFA_OUTSIDE_MODULE;
    if (tr == TR_LAG || tr == TR_GRID) {
        if (!h_lag || (uintptr_t)d_el % unit) return SHAFA_OUTSIDE_MODULE;
        for (int i = 0; i < nblocks; ++i) {
            const u64 *g = h_lag + (size_t)i * nlags;
            if (!g[0] || h_off[i] % unit) return SHAFA_OUTSIDE_MODULE;
            for (uint32_t k = 1; k < nlags; ++k)     // 0: unused, and so is every slot behind it; else past the slot in front
                if (g[k] ? g[k] <= g[k - 1] : k + 1 < nlags && g[k + 1]) return SHAFA_OUTSIDE_MODULE;
        }
    }
    if (fq) {                                        // the _grid_quant entries' own, where the lags are checked
        if (fq->round) {                             // the _grid_round entries': widths and kept bits for steps and bounds
            if (!fq->h_mant || !fq->h_keep || !round_params_ok(unit, nblocks, fq->h_mant, fq->h_keep)) return SHAFA_OUTSIDE_MODULE;
        } else {
            if (!fq->h_step || (!merge && !fq->h_bound)) return SHAFA_OUTSIDE_MODULE;
            if (!field_params_ok(unit, nblocks, fq->h_step, merge ? nullptr : fq->h_bound)) return SHAFA_OUTSIDE_MODULE;
        }
        if ((!merge && !fq->d_outl_n) || !fq->h_outl_off || !fq->h_outl_count) return SHAFA_OUTSIDE_MODULE;
        for (int i = 0; !fq->d_outl && i < nblocks; ++i)
            if (fq->h_outl_count[i]) return SHAFA_OUTSIDE_MODULE;
    }
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    if (tr == TR_LAG)
        return planes_lag_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, unit, merge, (u8 *)d_el, h_off, h_cap, d_n,
                                     (u8 *)d_planes, h_plane_off, h_lag);
    if (tr == TR_GRID)
        return planes_grid_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, unit, merge, (u8 *)d_el, h_off, h_cap, d_n,
                                      (u8 *)d_planes, h_plane_off, nlags, h_lag, fq);
    if (tr == TR_RECORDS)
        return records_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, unit, merge, (u8 *)d_el, h_off, h_cap, d_n, (u8 *)d_planes,
                                  h_plane_off);
    if (tr == TR_DIFF)
        return planes_diff_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, unit, merge, (u8 *)d_el, h_off, h_cap, d_n,
                                      (u8 *)d_planes, h_plane_off);
    return planes_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, unit, merge, (u8 *)d_el, h_off, h_cap, d_n, (u8 *)d_planes,
                             h_plane_off, xr ? d_base : nullptr, xr ? h_base_off : nullptr);
}

int shafa_hipd_split_planes_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_PLANES, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes, h_plane_off);
}

int shafa_hipd_merge_planes_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_PLANES, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes, h_plane_off);
}

int shafa_hipd_split_planes_xor_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint8_t *d_base, const uint64_t *h_base_off,
                                    const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes, const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_XOR, b, stream, nblocks, elem, d_in, h_in_off, d_base, h_base_off, h_cap, d_n, d_planes, h_plane_off);
}

int shafa_hipd_merge_planes_xor_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                    const uint64_t *h_plane_off, const uint8_t *d_base, const uint64_t *h_base_off,
                                    const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_XOR, b, stream, nblocks, elem, d_out, h_out_off, d_base, h_base_off, h_cap, d_n, d_planes, h_plane_off);
}

int shafa_hipd_split_planes_diff_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                     const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                     const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_DIFF, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off);
}

int shafa_hipd_merge_planes_diff_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                     const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                     const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_DIFF, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off);
}

int shafa_hipd_split_planes_lag_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint64_t *h_lag,
                                    const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n,
                                    uint8_t *d_planes, const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_LAG, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lag);
}

int shafa_hipd_merge_planes_lag_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint64_t *h_lag,
                                    const uint8_t *d_planes, const uint64_t *h_plane_off, const uint64_t *h_cap,
                                    const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_LAG, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lag);
}

int shafa_hipd_split_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                     const uint64_t *h_lags, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                                     const uint64_t *d_n, uint8_t *d_planes, const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_GRID, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags);
}

int shafa_hipd_merge_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                     const uint64_t *h_lags, const uint8_t *d_planes, const uint64_t *h_plane_off,
                                     const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_GRID, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags);
}

// the error-bounded fields: the _grid entries with a quantiser in the split and a restorer behind the merge
int shafa_hipd_split_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const double *h_step, const double *h_bound, const uint8_t *d_in,
                                           const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                           const uint64_t *h_plane_off, uint64_t *d_outl, const uint64_t *h_outl_off,
                                           const uint64_t *h_outl_cap, uint64_t *d_outl_n)
{
    const FieldQuant fq = {h_step, h_bound, d_outl, h_outl_off, h_outl_cap, d_outl_n};
    return transpose_dev(false, TR_GRID, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags, &fq);
}

int shafa_hipd_merge_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const double *h_step, const uint8_t *d_planes,
                                           const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n,
                                           const uint64_t *d_outl, const uint64_t *h_outl_off, const uint64_t *h_outl_n,
                                           uint8_t *d_out, const uint64_t *h_out_off)
{
    const FieldQuant fq = {h_step, nullptr, (u64 *)d_outl, h_outl_off, h_outl_n, nullptr};
    return transpose_dev(true, TR_GRID, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags, &fq);
}

// point-wise relative bounds: the _grid_quant entries with the rounding of the mantissa for the quantiser
int shafa_hipd_split_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep, const uint8_t *d_in,
                                           const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                           const uint64_t *h_plane_off, uint64_t *d_outl, const uint64_t *h_outl_off,
                                           const uint64_t *h_outl_cap, uint64_t *d_outl_n)
{
    const FieldQuant fq = {nullptr, nullptr, d_outl, h_outl_off, h_outl_cap, d_outl_n, true, h_mant, h_keep};
    return transpose_dev(false, TR_GRID, b, stream, nblocks, elem, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags, &fq);
}

int shafa_hipd_merge_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep,
                                           const uint8_t *d_planes, const uint64_t *h_plane_off, const uint64_t *h_cap,
                                           const uint64_t *d_n, const uint64_t *d_outl, const uint64_t *h_outl_off,
                                           const uint64_t *h_outl_n, uint8_t *d_out, const uint64_t *h_out_off)
{
    const FieldQuant fq = {nullptr, nullptr, (u64 *)d_outl, h_outl_off, h_outl_n, nullptr, true, h_mant, h_keep};
    return transpose_dev(true, TR_GRID, b, stream, nblocks, elem, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off, h_lags, nlags, &fq);
}

// beside transpose_dev: its TR_GRID checks in its order without a plane side.  GH_PLAIN: shafa_hipd_hist_planes_grid_dev, any
// elem and a row of zeros allowed (plain planes).  GH_QUANT: shafa_hipd_hist_planes_grid_quant_dev, elem 4 or 8, the _grid_quant
// split's rows (none of zeros) and, where the lags are checked, its steps and bounds and d_outl_n.  GH_ROUND:
// shafa_hipd_hist_planes_grid_round_dev, the same at elem 2, 4 or 8 with h_mant and h_keep for the steps and bounds
enum GridHist { GH_PLAIN, GH_QUANT, GH_ROUND };
static int grid_hist_dev(GridHist kind, shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                         const uint64_t *h_lags, const double *h_step, const double *h_bound, const uint8_t *d_in,
                         const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_freq, uint64_t *d_outl_n,
                         const uint32_t *h_mant = nullptr, const uint32_t *h_keep = nullptr)
{
    const bool quant = kind != GH_PLAIN;
    if (!b || !d_in || !d_freq || !d_n) return SHAFA_OUTSIDE_MODULE;
    if (nlags < 1 || nlags > SHAFA_PLANES_GRID_LAGS) return SHAFA_OUTSIDE_MODULE;
    const bool elem_ok = elem == 4 || elem == 8 || (elem == 2 && kind != GH_QUANT) || (elem == 1 && kind == GH_PLAIN);
    if (!elem_ok) return SHAFA_OUTSIDE_MODULE;
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_cap) return SHAFA_OUTSIDE_MODULE;
    u64 bytes = 0;
    for (int i = 0; i < nblocks; ++i) {
        if (h_cap[i] > ~0ull / elem || bytes + h_cap[i] * elem < bytes) return SHAFA_LACK_OF_MEMORY;
        bytes += h_cap[i] * elem;
    }
    if (tile_count(nblocks, h_cap, SHAFA_PLANES_TILE) < nblocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_in_off || !h_lags || (uintptr_t)d_in % elem) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i) {
        const u64 *g = h_lags + (size_t)i * nlags;
        if (h_in_off[i] % elem || (quant && !g[0])) return SHAFA_OUTSIDE_MODULE;
        for (uint32_t k = 1; k < nlags; ++k)         // the _grid entries' rows, or all zeros: a 0 has only zeros behind it
            if (g[k] && (!g[k - 1] || g[k] <= g[k - 1])) return SHAFA_OUTSIDE_MODULE;
    }
    if (kind == GH_QUANT && (!h_step || !h_bound || !field_params_ok(elem, nblocks, h_step, h_bound))) return SHAFA_OUTSIDE_MODULE;
    if (kind == GH_ROUND && (!h_mant || !h_keep || !round_params_ok(elem, nblocks, h_mant, h_keep))) return SHAFA_OUTSIDE_MODULE;
    if (quant && !d_outl_n) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    const FieldQuant fq = {h_step, h_bound, nullptr, nullptr, nullptr, d_outl_n, kind == GH_ROUND, h_mant, h_keep};
    return planes_grid_hist_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, elem, d_in, h_in_off, h_cap, d_n, nlags, h_lags,
                                       quant ? &fq : nullptr, d_freq);
}

int shafa_hipd_hist_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                    const uint64_t *h_lags, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                                    const uint64_t *d_n, uint64_t *d_freq)
{
    return grid_hist_dev(GH_PLAIN, b, stream, nblocks, elem, nlags, h_lags, nullptr, nullptr, d_in, h_in_off, h_cap, d_n, d_freq, nullptr);
}

int shafa_hipd_hist_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                          const uint64_t *h_lags, const double *h_step, const double *h_bound, const uint8_t *d_in,
                                          const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_freq,
                                          uint64_t *d_outl_n)
{
    return grid_hist_dev(GH_QUANT, b, stream, nblocks, elem, nlags, h_lags, h_step, h_bound, d_in, h_in_off, h_cap, d_n, d_freq, d_outl_n);
}

int shafa_hipd_hist_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                          const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep, const uint8_t *d_in,
                                          const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_freq,
                                          uint64_t *d_outl_n)
{
    return grid_hist_dev(GH_ROUND, b, stream, nblocks, elem, nlags, h_lags, nullptr, nullptr, d_in, h_in_off, h_cap, d_n, d_freq, d_outl_n,
                         h_mant, h_keep);
}

// error statistics.  The capacities of a call's blocks in elements: their bytes fit 64 bits and their tiles 31
static bool error_caps_ok(uint32_t elem, int nblocks, const uint64_t *h_cap)
{
    u64 bytes = 0;
    for (int i = 0; i < nblocks; ++i) {
        if (h_cap[i] > ~0ull / elem || bytes + h_cap[i] * elem < bytes) return false;
        bytes += h_cap[i] * elem;
    }
    return tile_count(nblocks, h_cap, SHAFA_PLANES_TILE) == nblocks;
}

// the fused entries: grid_hist_dev's checks in its order without the lags, the record for d_freq and d_outl_n
static int error_fused_dev(ErrorArgs e, shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                           const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_stat)
{
    if (!b || !d_in || !d_n) return SHAFA_OUTSIDE_MODULE;
    if (elem != 4 && elem != 8 && !(elem == 2 && e.src == ERR_ROUND)) return SHAFA_OUTSIDE_MODULE;
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_cap) return SHAFA_OUTSIDE_MODULE;
    if (!error_caps_ok(elem, nblocks, h_cap)) return SHAFA_LACK_OF_MEMORY;
    if (!h_in_off || (uintptr_t)d_in % elem) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (h_in_off[i] % elem) return SHAFA_OUTSIDE_MODULE;
    if (e.src == ERR_QUANT && (!e.h_step || !e.h_bound || !field_params_ok(elem, nblocks, e.h_step, e.h_bound))) return SHAFA_OUTSIDE_MODULE;
    if (e.src == ERR_ROUND && (!e.h_mant || !e.h_keep || !round_params_ok(elem, nblocks, e.h_mant, e.h_keep))) return SHAFA_OUTSIDE_MODULE;
    if (!d_stat) return SHAFA_OUTSIDE_MODULE;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return planes_error_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, elem, e, d_in, h_in_off, h_cap, d_n, d_stat);
}

int shafa_hipd_error_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const double *h_step,
                               const double *h_bound, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                               const uint64_t *d_n, uint64_t *d_stat)
{
    const ErrorArgs e = {ERR_QUANT, nullptr, nullptr, h_step, h_bound, nullptr, nullptr, nullptr, nullptr};
    return error_fused_dev(e, b, stream, nblocks, elem, d_in, h_in_off, h_cap, d_n, d_stat);
}

int shafa_hipd_error_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint32_t *h_mant,
                               const uint32_t *h_keep, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                               const uint64_t *d_n, uint64_t *d_stat)
{
    const ErrorArgs e = {ERR_ROUND, h_mant, h_keep, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return error_fused_dev(e, b, stream, nblocks, elem, d_in, h_in_off, h_cap, d_n, d_stat);
}

int shafa_hipd_error_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint32_t *h_mant, const double *h_abs,
                         const double *h_rel, const uint8_t *d_a, const uint64_t *h_a_off, const uint64_t *h_cap,
                         const uint64_t *d_n, const uint8_t *d_ref, const uint64_t *h_ref_off, uint64_t *d_stat)
{
    if (!d_a || !d_ref || ((uintptr_t)d_a & 15)) return SHAFA_OUTSIDE_MODULE;
    if (elem != 2 && elem != 4 && elem != 8) return SHAFA_OUTSIDE_MODULE;
    int rc;
    if (!size_pass_check((Batch *)b, nblocks, h_a_off, h_cap, d_n, d_n, &rc)) return rc;    // compare_dev's side a; d_stat: below
    if (!error_caps_ok(elem, nblocks, h_cap)) return SHAFA_LACK_OF_MEMORY;
    if (!h_ref_off || (uintptr_t)d_ref % elem) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (h_ref_off[i] % elem) return SHAFA_OUTSIDE_MODULE;
    if (!h_mant || !round_params_ok(elem, nblocks, h_mant, h_mant)) return SHAFA_OUTSIDE_MODULE;     // the widths alone: keep = mant
    if (!d_stat || !h_abs || !h_rel) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (!(h_abs[i] >= 0) || !(h_rel[i] >= 0) || std::isinf(h_rel[i])) return SHAFA_OUTSIDE_MODULE;
    if ((rc = batch_enter((Batch *)b, (hipStream_t)stream))) return rc;
    const ErrorArgs e = {ERR_PAIR, h_mant, nullptr, nullptr, nullptr, h_abs, h_rel, d_ref, h_ref_off};
    return planes_error_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, elem, e, d_a, h_a_off, h_cap, d_n, d_stat);
}

int shafa_hipd_split_records_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t width, const uint8_t *d_in,
                                 const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                 const uint64_t *h_plane_off)
{
    return transpose_dev(false, TR_RECORDS, b, stream, nblocks, width, d_in, h_in_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off);
}

int shafa_hipd_merge_records_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t width, const uint8_t *d_planes,
                                 const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                 const uint64_t *h_out_off)
{
    return transpose_dev(true, TR_RECORDS, b, stream, nblocks, width, d_out, h_out_off, nullptr, nullptr, h_cap, d_n, d_planes,
                         h_plane_off);
}

// span: a power of two, 256 .. 8192; flags: SHAFA_SEEK_SF / SHAFA_SEEK_RLE only
static bool seek_shape_ok(uint32_t span, int flags)
{
    return span >= 256 && span <= 8192 && (span & (span - 1)) == 0 && (flags & ~(SHAFA_SEEK_SF | SHAFA_SEEK_RLE)) == 0;
}

int shafa_hipd_seek_index_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                              const uint64_t *h_in_cap, const uint64_t *d_in_n, const shafa_code_table *d_tables, uint32_t span,
                              int flags, const uint64_t *h_ckpt_first, uint64_t *d_ckpt, uint32_t *d_status, uint64_t *d_out_n)
{
    if (!b || !d_in || !d_in_n || !d_ckpt || !d_status || !d_out_n) return SHAFA_OUTSIDE_MODULE;
    if (!seek_shape_ok(span, flags) || ((flags & SHAFA_SEEK_SF) && !d_tables)) return SHAFA_OUTSIDE_MODULE;
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (!h_in_off || !h_in_cap || !h_ckpt_first || ((uintptr_t)d_in & 15)) return SHAFA_OUTSIDE_MODULE;
    const int fit = tile_count(nblocks, h_in_cap, span);       // block by block: the offset, then the spans so far
    for (int i = 0; i < nblocks && i <= fit; ++i)
        if (h_in_off[i] & 15) return SHAFA_OUTSIDE_MODULE;
    if (fit < nblocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return seek_index_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_in, h_in_off, h_in_cap, d_in_n,
                                 (flags & SHAFA_SEEK_SF) ? d_tables : nullptr, span, flags, h_ckpt_first, d_ckpt, d_status, d_out_n);
}

int shafa_hipd_read_spans_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_file, uint64_t file_n,
                              const uint64_t *h_pay_off, const uint64_t *h_pay_n, const uint64_t *h_n_symbols,
                              const uint64_t *h_ckpt_first, const shafa_code_table *d_tables, uint32_t span, int flags,
                              const uint64_t *d_ckpt, int nitems, const int *h_item_block, const uint64_t *h_item_first,
                              const uint64_t *h_item_last, const uint64_t *h_item_lo, const uint64_t *h_item_hi,
                              const uint64_t *h_item_dst, uint8_t *d_out, uint64_t out_n)
{
    if (!b || !d_ckpt || !d_out || (!d_file && file_n)) return SHAFA_OUTSIDE_MODULE;
    if (!seek_shape_ok(span, flags) || ((flags & SHAFA_SEEK_SF) && !d_tables)) return SHAFA_OUTSIDE_MODULE;
    if (nitems <= 0) return SHAFA_SUCCESS;
    if (nitems > ((Batch *)b)->max_blocks || nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (nblocks <= 0 || !h_pay_off || !h_pay_n || !h_n_symbols || !h_ckpt_first || !h_item_block || !h_item_first ||
        !h_item_last || !h_item_lo || !h_item_hi || !h_item_dst)
        return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nblocks; ++i)
        if (h_pay_n[i] > file_n || h_pay_off[i] > file_n - h_pay_n[i] || h_pay_n[i] >= (1ull << 45)) return SHAFA_OUTSIDE_MODULE;
    for (int i = 0; i < nitems; ++i) {
        const int blk = h_item_block[i];
        if (blk < 0 || blk >= nblocks) return SHAFA_OUTSIDE_MODULE;
        const u64 ns = h_n_symbols[blk], nck = ns ? ns / span + (ns % span != 0) : 1;
        if (h_item_first[i] > h_item_last[i] || h_item_last[i] >= nck || h_item_last[i] > 0xFFFFFFFFull) return SHAFA_OUTSIDE_MODULE;
        if (h_item_lo[i] > h_item_hi[i] || h_item_dst[i] > out_n || h_item_hi[i] - h_item_lo[i] > out_n - h_item_dst[i])
            return SHAFA_OUTSIDE_MODULE;
    }
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return read_spans_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_file, h_pay_off, h_pay_n, h_n_symbols, h_ckpt_first,
                                 (flags & SHAFA_SEEK_SF) ? d_tables : nullptr, span, flags, d_ckpt, nitems, h_item_block,
                                 h_item_first, h_item_last, h_item_lo, h_item_hi, h_item_dst, d_out);
}

int shafa_hipd_sf_encoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint64_t *d_freq,
                                   const shafa_code_table *d_tables, uint64_t *d_out_n)
{
    if (!b || !d_freq || !d_tables || !d_out_n) return SHAFA_OUTSIDE_MODULE;
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > ((Batch *)b)->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if (int rc = batch_enter((Batch *)b, (hipStream_t)stream)) return rc;
    return sfesize_launch_dev((Batch *)b, (hipStream_t)stream, nblocks, d_freq, d_tables, d_out_n);
}

}  // extern "C"

// the call itself (not a block) failed: no block has a result — every block reports the call's code
static int finish_failed(Batch *b, int nblocks, int *h_block_err, int rc)
{
    for (int i = 0; b && i < nblocks && i < b->max_blocks; ++i) {
        if (h_block_err) h_block_err[i] = rc;
        b->h_hosterr[i] = 0;
    }
    return rc;
}

int batch_finish(Batch *b, hipStream_t st, int nblocks, int *h_block_err, bool *call_failed)
{
    if (call_failed) *call_failed = true;
    if (int rc = batch_enter(b, st)) return finish_failed(b, nblocks, h_block_err, rc);
    if (nblocks > b->max_blocks) nblocks = b->max_blocks;
    if (nblocks < 0) nblocks = 0;
    hipError_t e = hipSuccess;
    if (nblocks) {
        e = hipMemcpyAsync(b->h_err, b->d_err, (size_t)nblocks * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemsetAsync(b->d_err, 0, (size_t)nblocks * sizeof(int), st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return finish_failed(b, nblocks, h_block_err, shafa_set_hip_error(e, "shafa_hipd_finish"));
    if (call_failed) *call_failed = false;
    batch_stage_retire(b, st);
    if (b->copy_st) batch_stage_retire(b, b->copy_st);  // `st` waited for every parameter copy: they are through as well
    int first = SHAFA_SUCCESS;
    for (int i = 0; i < nblocks; ++i) {
        const int e = b->h_hosterr[i] ? b->h_hosterr[i] : b->h_err[i];
        b->h_hosterr[i] = 0;
        if (h_block_err) h_block_err[i] = e;
        if (!first && e) first = e;
    }
    if (first == SHAFA_DEVICE_ERROR)
        snprintf(g_last_error, sizeof(g_last_error), "kernel reported a lost predecessor tile (spin bound hit)");
    return first;
}

extern "C" {

int shafa_hipd_finish(shafa_hipd_batch *hb, void *stream, int nblocks, int *h_block_err)
{
    return batch_finish((Batch *)hb, (hipStream_t)stream, nblocks, h_block_err, nullptr);
}

int shafa_hipd_gen_bytes(void *stream, uint64_t seed, uint64_t first_index, const uint8_t *d_map65536,
                         uint8_t *d_out, size_t n)
{
    return gen_launch((hipStream_t)stream, seed, first_index, d_map65536, d_out, n);
}

// ------------------------------------------------------------------------------------------------
// layer 1: host buffers, one block per call, synchronous
// ------------------------------------------------------------------------------------------------
static struct {
    bool ready;
    int device;
    hipStream_t stream;
    Batch *batch;
    u8 *d_a; size_t a_bytes;     // input staging on the device
    u8 *d_b; size_t b_bytes;     // output staging on the device
    u64 *d_small;                // 256 u64 histogram + 1 u64 size
} g;

static int g_devs[64];
static int g_ndevs = 0;                     // 0: layer 3 uses the layer-1 device only

// Layer 1 keeps ONE stream, batch context and pair of staging buffers per process.  The reference calls the functions
// layer 1 replaces from one thread per block at the same time (multithread.c:70-87 with c.c:411, d.c:735), so every
// layer-1 entry point takes this lock for its whole duration: calls from several threads are safe and run one after the
// other on the GPU (a block's kernels fill the device anyway; overlap of copies and kernels is what layer 3 is for).
static std::recursive_mutex g_l1_mu;
#define L1_ENTER()                                   \
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu); \
    int rc = lazy_init();                            \
    if (rc) return rc;                               \
    DeviceGuard l1_dev(g.device)

static int ensure_dev(u8 **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return SHAFA_SUCCESS;
    if (*p) { HIP_TRY(hipFree(*p)); *p = nullptr; *cap = 0; }
    const size_t want = ((bytes + (bytes >> 3) + 4096) + 255) & ~(size_t)255;
    HIP_TRY(hipMalloc((void **)p, want));
    *cap = want;
    return SHAFA_SUCCESS;
}

int shafa_hip_init(int device)
{
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu);
    if (g.ready && g.device == device) return SHAFA_SUCCESS;
    if (g.ready) shafa_hip_shutdown();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        snprintf(g_last_error, sizeof(g_last_error), "no HIP device visible");
        return SHAFA_DEVICE_ERROR;
    }
    if (device < 0 || device >= n) return SHAFA_OUTSIDE_MODULE;
    DeviceGuard dg(device);                      // the caller's current device is left as it was
    if (const char *e = getenv("SHAFA_SF_ENCODE_ONE_PASS_MIN_BLOCKS")) shafa_hip_set_option("sf_encode_one_pass_min_blocks", atol(e));
    if (const char *e = getenv("SHAFA_SF_DECODE_SPECULATE")) shafa_hip_set_option("sf_decode_speculate", atol(e));
    HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    shafa_hipd_batch *bh = nullptr;
    int rc = shafa_hipd_batch_create(1, (size_t)1 << 27, &bh);
    if (rc) return rc;
    g.batch = (Batch *)bh;
    HIP_TRY(hipMalloc((void **)&g.d_small, 257 * sizeof(u64)));
    g.device = device;
    g.ready = true;
    return SHAFA_SUCCESS;
}

void shafa_hip_shutdown(void)
{
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu);
    if (!g.ready) return;
    DeviceGuard dg(g.device);
    hipDeviceSynchronize();
    shafa_hipd_batch_destroy((shafa_hipd_batch *)g.batch);
    if (g.d_a) hipFree(g.d_a);
    if (g.d_b) hipFree(g.d_b);
    if (g.d_small) hipFree(g.d_small);
    hipStreamDestroy(g.stream);
    memset(&g, 0, sizeof(g));
    g_ndevs = 0;
}


int shafa_hip_init_devices(const int *devices, int n_devices)
{
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        snprintf(g_last_error, sizeof(g_last_error), "no HIP device visible");
        return SHAFA_DEVICE_ERROR;
    }
    if (n_devices < 0 || n_devices > 64 || (n_devices && !devices)) return SHAFA_OUTSIDE_MODULE;
    int list[64], m = 0;
    if (n_devices == 0) { for (; m < n && m < 64; ++m) list[m] = m; }
    else for (; m < n_devices; ++m) { if (devices[m] < 0 || devices[m] >= n) return SHAFA_OUTSIDE_MODULE; list[m] = devices[m]; }
    int rc = shafa_hip_init(list[0]);
    if (rc) return rc;
    memcpy(g_devs, list, sizeof(int) * (size_t)m);
    g_ndevs = m;
    return SHAFA_SUCCESS;
}

int shafa_hip_devices(void) { return g_ndevs ? g_ndevs : 1; }

static int lazy_init(void)
{
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu);
    return g.ready ? SHAFA_SUCCESS : shafa_hip_init(0);
}

static int upload(const uint8_t *in, size_t n)
{
    int rc = ensure_dev(&g.d_a, &g.a_bytes, n + 64);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(g.d_a, in, n, hipMemcpyHostToDevice, g.stream));
    return SHAFA_SUCCESS;
}

int shafa_hip_hist256(const uint8_t *in, size_t n, uint64_t freq[256])
{
    L1_ENTER();
    if ((rc = upload(in, n))) return rc;
    const u64 off[1] = {0}, len[1] = {n};
    if ((rc = hist_launch(g.batch, g.stream, 1, g.d_a, off, len, g.d_small))) return rc;
    HIP_TRY(hipMemcpyAsync(freq, g.d_small, 256 * sizeof(u64), hipMemcpyDeviceToHost, g.stream));
    return shafa_hipd_finish((shafa_hipd_batch *)g.batch, g.stream, 1, nullptr);
}

int shafa_hip_rle_encode(const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_n,
                         uint64_t *freq_out)
{
    L1_ENTER();
    if (out_cap < 2 * n + 3) return SHAFA_LACK_OF_MEMORY;      // f.c:244 worst case
    if ((rc = upload(in, n))) return rc;
    const size_t cap = (2 * n + 3 + 15) & ~(size_t)15;
    if ((rc = ensure_dev(&g.d_b, &g.b_bytes, cap))) return rc;
    const u64 ioff[1] = {0}, ilen[1] = {n}, ooff[1] = {0}, ocap[1] = {cap};
    if ((rc = rleenc_launch(g.batch, g.stream, 1, g.d_a, ioff, ilen, g.d_b, ooff, ocap, g.d_small + 256,
                            freq_out ? g.d_small : nullptr))) return rc;
    u64 sz = 0;
    HIP_TRY(hipMemcpyAsync(&sz, g.d_small + 256, sizeof(u64), hipMemcpyDeviceToHost, g.stream));
    if (freq_out) HIP_TRY(hipMemcpyAsync(freq_out, g.d_small, 256 * sizeof(u64), hipMemcpyDeviceToHost, g.stream));
    rc = shafa_hipd_finish((shafa_hipd_batch *)g.batch, g.stream, 1, nullptr);
    if (rc) return rc;
    if (sz > out_cap) return SHAFA_LACK_OF_MEMORY;
    if (sz) HIP_TRY(hipMemcpy(out, g.d_b, sz, hipMemcpyDeviceToHost));
    *out_n = (size_t)sz;
    return SHAFA_SUCCESS;
}

int shafa_hip_sf_encode(const uint8_t *in, size_t n, const shafa_code_table *table,
                        uint8_t *out, size_t out_cap, size_t *out_n)
{
    L1_ENTER();
    if ((rc = upload(in, n))) return rc;
    const size_t cap = (out_cap + 15) & ~(size_t)15;
    if ((rc = ensure_dev(&g.d_b, &g.b_bytes, cap + 16))) return rc;
    // the device region is the caller's capacity (rounded down to keep the bound exact)
    const u64 ioff[1] = {0}, ilen[1] = {n}, ooff[1] = {0}, ocap[1] = {out_cap};
    if ((rc = sfenc_launch(g.batch, g.stream, 1, g.d_a, ioff, ilen, table, g.d_b, ooff, ocap, g.d_small + 256))) return rc;
    u64 sz = 0;
    HIP_TRY(hipMemcpyAsync(&sz, g.d_small + 256, sizeof(u64), hipMemcpyDeviceToHost, g.stream));
    rc = shafa_hipd_finish((shafa_hipd_batch *)g.batch, g.stream, 1, nullptr);
    if (rc) return rc;
    if (sz > out_cap) return SHAFA_LACK_OF_MEMORY;
    if (sz) HIP_TRY(hipMemcpy(out, g.d_b, sz, hipMemcpyDeviceToHost));
    *out_n = (size_t)sz;
    return SHAFA_SUCCESS;
}

int shafa_hip_sf_decode(const uint8_t *in, size_t in_n, const shafa_code_table *table,
                        uint8_t *out, size_t n_symbols)
{
    L1_ENTER();
    if ((rc = upload(in, in_n))) return rc;
    if ((rc = ensure_dev(&g.d_b, &g.b_bytes, n_symbols + 64))) return rc;
    const u64 ioff[1] = {0}, ilen[1] = {in_n}, ooff[1] = {0}, ns[1] = {n_symbols};
    if ((rc = sfdec_launch(g.batch, g.stream, 1, g.d_a, ioff, ilen, table, ns, g.d_b, ooff))) return rc;
    rc = shafa_hipd_finish((shafa_hipd_batch *)g.batch, g.stream, 1, nullptr);
    if (rc) return rc;
    if (n_symbols) HIP_TRY(hipMemcpy(out, g.d_b, n_symbols, hipMemcpyDeviceToHost));
    return SHAFA_SUCCESS;
}

int shafa_hip_rle_decode(const uint8_t *in, size_t in_n, uint8_t *out, size_t out_cap, size_t *out_n)
{
    L1_ENTER();
    if ((rc = upload(in, in_n))) return rc;
    size_t cap = out_cap < SHAFA_RLE_DECODE_MAX ? out_cap : SHAFA_RLE_DECODE_MAX;
    if ((rc = ensure_dev(&g.d_b, &g.b_bytes, cap + 64))) return rc;
    const u64 ioff[1] = {0}, ilen[1] = {in_n}, ooff[1] = {0}, ocap[1] = {cap};
    if ((rc = rledec_launch(g.batch, g.stream, 1, g.d_a, ioff, ilen, g.d_b, ooff, ocap, g.d_small + 256))) return rc;
    u64 sz = 0;
    HIP_TRY(hipMemcpyAsync(&sz, g.d_small + 256, sizeof(u64), hipMemcpyDeviceToHost, g.stream));
    rc = shafa_hipd_finish((shafa_hipd_batch *)g.batch, g.stream, 1, nullptr);
    if (rc) return rc;
    if (sz) HIP_TRY(hipMemcpy(out, g.d_b, sz, hipMemcpyDeviceToHost));
    *out_n = (size_t)sz;
    return SHAFA_SUCCESS;
}

}  // extern "C"

int api_lazy_init() { return lazy_init(); }     // layer 3 (pipe.hip)
// device of slot `slot` of a pipe with n_slots slots: the selected devices in turn, but no more devices than the pipe can
// keep busy with three blocks in flight each (a two-block file on an eight-GPU node opens one context, not eight)
int api_pipe_device(int slot, int n_slots)
{
    std::lock_guard<std::recursive_mutex> l1_lock(g_l1_mu);
    if (!g_ndevs) return g.device;
    int used = (n_slots + 2) / 3;
    if (used < 1) used = 1;
    if (used > g_ndevs) used = g_ndevs;
    return g_devs[slot % used];
}
