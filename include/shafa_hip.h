/*
 * shafa_hip.h — C-ABI of libshafa_hip.so: the MI355X (gfx950) implementation of Shafa's per-block
 * hot path (Modules F, C, D).  Plain C, plain pointers and sizes, no C++/torch types.
 *
 * The reference (Fytex/Shafa-CD) has no plugin/FFI interface; its seam is the per-block
 * `process` callback handed to multithread_create (utils/multithread.h:45) and the direct calls
 * in f.c.  Each entry point below replaces one of those static functions (cited per function,
 * paths relative to /root/reference/src/modules/).  Return values are the reference's
 * _modules_error numbers (utils/errors.h:5-16) plus SHAFA_DEVICE_ERROR.
 *
 * Two layers:
 *   1. host-buffer, one block per call, synchronous  (shafa_hip_*)   — what the C host's
 *      f/c/d drivers call in place of f.c:248,310,325, c.c:411, d.c:342,735.
 *   2. device-resident, many blocks per launch, asynchronous on a caller stream (shafa_hipd_*)
 *      — used by the streaming drivers, bench.py and the multi-GPU sharding; every pointer named
 *      d_* is a DEVICE pointer, every h_* a HOST pointer.
 *
 * Threading.  The reference calls the functions layer 1 replaces from one pthread per block at the same time
 * (utils/multithread.c:70-87 starts `process` per block; c.c:411 compress_to_buffer, d.c:735 process_shafa_decomp), so
 * LAYER 1 IS THREAD-SAFE: every shafa_hip_* entry point may be called from any number of host threads concurrently.
 * Layer 1 keeps one stream and one pair of staging buffers per process and serialises the calls on an internal lock
 * (one block's kernels fill the GPU; overlap of copies, kernels and I/O is what layer 3 is for).
 * Layers 2 and 3: a batch / a pipe is used by one thread at a time; different batches and pipes may be used from different
 * threads concurrently.  A batch serves one stream at a time: a launch on another stream first waits for the batch's
 * previous stream.  The calling thread's current HIP device must be the batch's device (the one current at
 * shafa_hipd_batch_create) for layer-2 calls; layer 1 and layer 3 select their devices themselves and NO entry point
 * leaves the calling thread's current device changed.  shafa_hip_set_option() and shafa_hip_init*() are configuration:
 * call them while no other call is in flight.  shafa_hip_last_error() is per calling thread.  A decode call of 16 blocks
 * or more prepares its tables on up to seven short-lived helper threads of its own (joined before the call returns).
 * No entry point throws or exits.
 */
#ifndef SHAFA_HIP_H
#define SHAFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHAFA_HIP_ABI_VERSION 8

/* utils/errors.h:5-16 (_modules_error), same numbers */
enum shafa_error {
    SHAFA_SUCCESS = 0,
    SHAFA_OUTSIDE_MODULE = 1,
    SHAFA_LACK_OF_MEMORY = 2,
    SHAFA_FILE_INACCESSIBLE = 3,
    SHAFA_FILE_UNRECOGNIZABLE = 4,
    SHAFA_FILE_STREAM_FAILED = 5,
    SHAFA_FILE_TOO_SMALL = 6,
    SHAFA_THREAD_CREATION_FAILED = 7,
    SHAFA_THREAD_TERMINATION_FAILED = 8,
    SHAFA_DEVICE_ERROR = 9            /* HIP runtime failure / no GPU; see shafa_hip_last_error() */
};

/* One block's Shannon-Fano table, the binary form of one "c0;c1;...;c255" .cod block
 * (t.c:353-361; parsed by c.c:115-177 and d.c:466-504): len[s] = code length in bits
 * (0 = symbol absent, max 255), bits[s] = the code MSB-first, zero padded. */
typedef struct shafa_code_table {
    uint8_t len[256];
    uint8_t bits[256][32];
} shafa_code_table;

/* RLE decode output limit of the reference: 64 MiB + 1 KiB (d.c:129-169). */
#define SHAFA_RLE_DECODE_MAX ((size_t)67108864 + 1024)

/* ------------------------------------------------------------------ lifecycle */
int shafa_hip_abi_version(void);
int shafa_hip_device_count(void);            /* 0 when no GPU is visible; never fails */
int shafa_hip_init(int device);              /* select device, create the library's stream/workspace */
/* Select the devices of the block pipeline (layer 3): slot i of every pipe created afterwards lives on
 * devices[i % n_devices] (its stream, buffers and kernels), so the blocks of one file are spread over the GPUs of the
 * node while the caller still retires them in order (multithread.c:70-87) — of a pipe with n_slots slots only the first
 * ceil(n_slots / 3) selected devices are used (three blocks in flight keep a GPU busy; a short file does not open a
 * context on every GPU).  Layers 1 and 2 use devices[0].
 * n_devices == 0 selects every visible device.  Returns SHAFA_OUTSIDE_MODULE for an invalid device number. */
int shafa_hip_init_devices(const int *devices, int n_devices);
int shafa_hip_devices(void);                 /* number of devices selected for layer 3 (1 until shafa_hip_init_devices) */
void shafa_hip_shutdown(void);
const char *shafa_hip_last_error(void);      /* text of the last SHAFA_DEVICE_ERROR */

/* Tuning knobs (no reference counterpart).  Unknown names return SHAFA_OUTSIDE_MODULE.
 *   "sf_encode_one_pass_min_blocks": a shafa_hipd_sf_encode launch with at least this many blocks of <= 16-bit
 *       codes takes the one-pass encoder, smaller launches the count/scan/pack kernels; 0 (default) = the measured crossovers: 6 blocks
 *       where the 1024-lane form runs (every code <= 16 bits since round 3), 80 for the 256-lane form.
 *   "sf_decode_speculate": 1 (default) lets blocks whose code re-synchronises take the speculative entry kernels of
 *       the Shannon-Fano decoder (verified exactly; falls back to the exact kernels per block), 0 = exact kernels only,
 *       2 = speculate for every block the kernels apply to, whatever its code (for tests of the fall-back).
 *   "sf_encode_lanes": 0 (default) = the widest workgroup whose windows fit the CU's LDS (1024 lanes, 32 KiB tiles, for
 *       codes of <= 12 bits; 256 lanes otherwise), 256 / 512 = that width.
 * Test knobs that force the fall-back kernels the library otherwise takes by itself (tests/test_gpu_codec.py):
 *   "sf_decode_path": 0 (default) = the fastest kernels the tables allow, 1 = one code per look-up as for incomplete
 *       codes, 2 = the generic byte-map kernels of codes longer than 32 bits.
 *   "rle_encode_general": 1 = every tile takes the per-element general RLE code (long runs, ragged tiles), 0 = by data.
 *   "rle_encode_one_pass": 0 only = the two-pass RLE kernels, the one form there is; 1 (the one-pass form, removed after
 *       DESIGN.md 3.3 measured it slower) returns SHAFA_OUTSIDE_MODULE.
 *   "sf_encode_window_bits": bits per symbol the 1024-lane encoder's LDS windows are sized for; 0 (default) = the launch's
 *       longest code, at most 12.  A tile that needs more is not placed: its block is flagged on the device and encoded
 *       again by the 256-lane form in the same call (what happens to 13..16-bit codes whose rare symbols fill a whole
 *       32 KiB tile); small values make ordinary data take that path.
 *   "rle_grid_rows": what one launch of the RLE encoder's and decoder's kernels may put on its grid, as (rows of the
 *       largest block) x (blocks): a call's blocks are launched in consecutive runs within it, a block above it alone (rows:
 *       a decoder input's 8 KiB tiles, an encoder input's pairs of 4 KiB tiles).  0 (default) = 2^22, v >= 1 = v (at most
 *       2^24 - 1), negative: SHAFA_OUTSIDE_MODULE.  Results do not depend on it; small values make small batches take
 *       several runs.
 * shafa_hip_init() reads the environment variables SHAFA_SF_ENCODE_ONE_PASS_MIN_BLOCKS and SHAFA_SF_DECODE_SPECULATE
 * once for the first two knobs. */
int shafa_hip_set_option(const char *name, long value);

/* ------------------------------------------------------------------ layer 1: host buffers, one block */

/* make_freq (f.c:63-79): 256-bin byte histogram, 64-bit bins. */
int shafa_hip_hist256(const uint8_t *in, size_t n, uint64_t freq[256]);

/* block_compression (f.c:29-55) [+ make_freq of the RLE bytes, f.c:310, when freq_out != NULL].
 * out_cap must be >= 2n+3 (f.c:244) or the worst case is refused with SHAFA_LACK_OF_MEMORY. */
int shafa_hip_rle_encode(const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_n,
                         uint64_t *freq_out /* [256] or NULL */);

/* compress_to_buffer + binary_coding (c.c:52-237): concatenate the block's codes MSB-first,
 * zero-pad the last byte; *out_n = ceil(bits/8).  A data symbol with an empty code in a table that
 * holds non-empty codes is SHAFA_FILE_UNRECOGNIZABLE; an all-empty table gives 0 bytes (c.c:156).
 * A block with both faults — such a symbol AND an output that does not fit out_cap — is SHAFA_FILE_UNRECOGNIZABLE
 * (the symbols are looked at first), whichever the device notices first. */
int shafa_hip_sf_encode(const uint8_t *in, size_t n, const shafa_code_table *table,
                        uint8_t *out, size_t out_cap, size_t *out_n);

/* create_tree + shafa_block_decompressor (d.c:466-551): decode exactly n_symbols symbols.
 * Malformed table / missing branch / exhausted input is SHAFA_FILE_UNRECOGNIZABLE. */
int shafa_hip_sf_decode(const uint8_t *in, size_t in_n, const shafa_code_table *table,
                        uint8_t *out, size_t n_symbols);

/* rle_block_decompressor (d.c:116-197); more than SHAFA_RLE_DECODE_MAX bytes of output is
 * SHAFA_FILE_UNRECOGNIZABLE (d.c:165-168), more than out_cap is SHAFA_LACK_OF_MEMORY, a {0, symbol, count} cut by the end
 * of the block is SHAFA_FILE_UNRECOGNIZABLE.  A block with several of these reports the one a front-to-back decoder stops at
 * (the first token whose end passes out_cap or the maximum; a cut triple comes last), independent of timing. */
int shafa_hip_rle_decode(const uint8_t *in, size_t in_n, uint8_t *out, size_t out_cap, size_t *out_n);

/* ------------------------------------------------------------------ layer 2: device buffers, batches
 *
 * A batch is nblocks independent blocks.  Block b's input is the h_in_n[b] bytes at
 * d_in + h_in_off[b]; its output region is the h_out_cap[b] bytes at d_out + h_out_off[b]
 * (all four are host arrays of nblocks entries; every offset must be a multiple of 16).
 * The offsets are 64-bit in every entry of this layer, h_thist_off, h_plane_off, h_dst_off and the payload places in d_off
 * included: a region may lie anywhere in a buffer of any size, past byte 2^32 too; only a block's own size is bounded.
 * Calls enqueue work on `stream` (a hipStream_t passed as void*; NULL = the null stream) and
 * return without synchronising; results in device memory are valid after the stream is synchronised.
 * shafa_hipd_finish() synchronises the stream and returns the batch's first error, filling the
 * optional host arrays.  shafa_hipd_compare_dev alone has a second operand that needs no alignment: the original a decoder's
 * output is checked against, read in place.
 */
typedef struct shafa_hipd_batch shafa_hipd_batch;

/* Allocate a reusable batch context (device workspace, pinned staging) for up to max_blocks blocks
 * of up to max_block_bytes input bytes each (for RLE/SF decode: of the LARGER of input and output).
 * The device workspace grows on demand and is kept: the largest users are RLE encode (about 0.26 bytes per input
 * byte of a launch) and SF decode (about 0.1 bytes per byte of stream; 0.35 on the exact path of codes that do not
 * re-synchronise). */
int shafa_hipd_batch_create(int max_blocks, size_t max_block_bytes, shafa_hipd_batch **out);
void shafa_hipd_batch_destroy(shafa_hipd_batch *b);

/* make_freq per block: d_freq[b*256 + s], 64-bit counts. */
int shafa_hipd_hist256(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                       const uint64_t *h_in_off, const uint64_t *h_in_n, uint64_t *d_freq);

/* Module T's core on the device (t.c:74-210, the rule set of host/sfcodes.c shafa_sf_build_codes): d_freq = nblocks x 256
 * counts (what shafa_hipd_hist256 / _rle_encode leave), d_tables = nblocks tables in DEVICE memory, bit-identical to the
 * host's for counts whose sum fits 64 bits (a block's own histogram always does; else SHAFA_OUTSIDE_MODULE for the block
 * and an empty table).  One workgroup per block.  shafa_hipd_sf_encode_dev and shafa_hipd_sf_decode_dev take these tables
 * as they lie, which makes F -> T -> C -> D host-free; shafa_hipd_sf_encode / _sf_decode take HOST tables. */
int shafa_hipd_sf_build_codes(shafa_hipd_batch *b, void *stream, int nblocks, const uint64_t *d_freq,
                              shafa_code_table *d_tables);

/* block_compression per block; d_out_n[b] = RLE size; d_freq (may be NULL) = histogram of the RLE bytes.  Any number of
 * blocks of any sizes up to the batch's: the launches are cut to fit the grid ("rle_grid_rows").  A block of 2^24 pairs of
 * 4 KiB tiles (128 GiB) or more: SHAFA_LACK_OF_MEMORY for the call, before any device work. */
int shafa_hipd_rle_encode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                          const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                          const uint64_t *h_out_off, const uint64_t *h_out_cap,
                          uint64_t *d_out_n, uint64_t *d_freq);

/* binary_coding per block; d_out_n[b] = ceil(bits/8). */
int shafa_hipd_sf_encode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                         const uint64_t *h_in_off, const uint64_t *h_in_n,
                         const shafa_code_table *h_tables, uint8_t *d_out, const uint64_t *h_out_off,
                         const uint64_t *h_out_cap, uint64_t *d_out_n);

/* ---- Tile histograms: Module F's by-product that lets Module C run without any tile waiting for another ----------------
 * The reference's F -> T -> C sequence reads a block three times: make_freq (f.c:63-79), then — with the codes of Module T —
 * binary_coding (c.c:52-83), whose output position of byte i depends on the code lengths of all bytes before it.  A caller
 * that keeps a block resident in HBM between F and C can hand C what F already saw: the histogram of every
 * SHAFA_TILE_BYTES (32 KiB) tile of the block, 256 x uint16_t per tile (a tile holds at most 32768 of one byte value),
 * shafa_hip_tile_hist_bytes(n) bytes for a block of n bytes, tile t's counts at offset 512 t.  With them the bit offset of
 * every tile in the encoded block is (tile histograms . code lengths), scanned — known BEFORE the encoder starts — and the
 * encoder is a one-shot grid of independent workgroups (sf_encode6.hip) instead of a chained scan.  The histograms depend
 * on the data only, not on the codes.  Block b's tile histograms live at d_tile_hist + h_tile_hist_off[b] (offsets
 * multiples of 16).  Results are identical to the entry points without `_tiles`; histograms that are not the block's own
 * are detected (SHAFA_OUTSIDE_MODULE for the block, nothing is written outside its output region). */
#define SHAFA_TILE_BYTES 32768
size_t shafa_hip_tile_hist_bytes(size_t n);

/* make_freq per block as shafa_hipd_hist256, plus the tile histograms. */
int shafa_hipd_hist256_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_n, uint64_t *d_freq,
                             uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off);

/* block_compression + make_freq of the RLE bytes as shafa_hipd_rle_encode (d_freq required), plus the tile histograms of
 * the RLE bytes: block b's region must hold shafa_hip_tile_hist_bytes(h_out_cap[b]) bytes.  SHAFA_LACK_OF_MEMORY as there. */
int shafa_hipd_rle_encode_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                                const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n,
                                uint64_t *d_freq, uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off);

/* binary_coding per block as shafa_hipd_sf_encode, given the tile histograms of the input blocks. */
int shafa_hipd_sf_encode_tiles(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_n, const shafa_code_table *h_tables,
                               const uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off, uint8_t *d_out,
                               const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n);

/* binary_coding per block as shafa_hipd_sf_encode[_tiles], with the block sizes AND the code tables in DEVICE memory: block b
 * encodes d_in_n[b] (<= h_in_cap[b]) bytes at d_in + h_in_off[b] with d_tables[b] (what shafa_hipd_sf_build_codes leaves);
 * d_tile_hist / h_tile_hist_off either both NULL or the blocks' tile histograms (regions sized for h_in_cap[b]).  Results —
 * bytes, d_out_n[b], the per-block codes of shafa_hipd_finish — equal those of shafa_hipd_sf_encode[_tiles] with the same
 * tables on the host and h_in_n = d_in_n.  d_in_n[b] > h_in_cap[b] is SHAFA_OUTSIDE_MODULE for block b (d_out_n[b] = 0).
 * Nothing is written outside a block's output region: an output that does not fit is SHAFA_LACK_OF_MEMORY, and
 * h_out_cap[b] = h_in_cap[b] * L / 8 + 16 always suffices for codes of at most L bits.
 * Enqueues only: d_tables and d_in_n are never read on the host, no device-to-host copy is issued and neither the stream
 * nor the device is synchronised — so rle_encode_tiles / hist256_tiles -> sf_build_codes -> sf_encode_dev -> one
 * shafa_hipd_finish compresses a batch with a single synchronisation.  The one exception is the batch's growth on demand
 * (device workspace, parameter buffers, staging), which depends on nblocks and h_in_cap only: once a call of the same
 * shape has been made on the batch, the call never waits.  NULL b, d_in_n or d_tables: SHAFA_OUTSIDE_MODULE. */
int shafa_hipd_sf_encode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                             const shafa_code_table *d_tables, const uint8_t *d_tile_hist, const uint64_t *h_tile_hist_off,
                             uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n);

/* shafa_block_decompressor per block: block b decodes h_n_symbols[b] symbols from the h_in_n[b]
 * bytes at d_in + h_in_off[b] into d_out + h_out_off[b] (which must hold h_n_symbols[b] bytes). */
int shafa_hipd_sf_decode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                         const uint64_t *h_in_off, const uint64_t *h_in_n,
                         const shafa_code_table *h_tables, const uint64_t *h_n_symbols,
                         uint8_t *d_out, const uint64_t *h_out_off);

/* rle_block_decompressor per block; d_out_n[b] = decoded size.  Any number of blocks of any sizes up to the batch's: the
 * launches are cut to fit the grid ("rle_grid_rows").  A block of 2^24 tiles of 8 KiB (128 GiB) or more: SHAFA_LACK_OF_MEMORY
 * for the call, before any device work. */
int shafa_hipd_rle_decode(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                          const uint64_t *h_in_off, const uint64_t *h_in_n, uint8_t *d_out,
                          const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n);

/* shafa_hipd_sf_decode with the stream sizes, the symbol counts AND the code tables in DEVICE memory: block b decodes
 * d_n_symbols[b] symbols from the d_in_n[b] (<= h_in_cap[b]) bytes at d_in + h_in_off[b] with d_tables[b] (what
 * shafa_hipd_sf_build_codes leaves) into d_out + h_out_off[b].  Bytes and the per-block codes of shafa_hipd_finish equal
 * those of shafa_hipd_sf_decode with the same tables on the host, h_in_n = d_in_n and h_n_symbols = d_n_symbols —
 * malformed tables, empty streams and damaged streams included.  d_in_n[b] > h_in_cap[b] or d_n_symbols[b] > h_out_cap[b]
 * is SHAFA_OUTSIDE_MODULE for block b and nothing is written to its region; nothing is ever written outside
 * [h_out_off[b], h_out_off[b] + h_out_cap[b]).
 * Memory rule: a block whose codes have at most 32 bits never fails for want of memory.  Codes of 33..64 bits have one slot
 * per call, sized for max(h_in_cap): it goes to the first block by index with such a code, d_n_symbols > 0, d_in_n > 0
 * and both sizes within its capacities (a malformed table counts too); later blocks with codes of 33..64 bits, and every
 * block with a code of more than 64 bits, are SHAFA_LACK_OF_MEMORY, nothing written (malformed tables and the capacity
 * checks report first).  The device workspace is 1.35 bytes per byte of sum(h_in_cap), plus 2.1 bytes per byte of
 * max(h_in_cap), plus 187 KiB per block, plus 128 KiB.
 * Enqueues only: d_tables, d_in_n and d_n_symbols are never read on the host, no device-to-host copy is issued and
 * neither the stream nor the device is synchronised, as for shafa_hipd_sf_encode_dev (the same exception: the batch's
 * growth, from nblocks and the capacities).  The options sf_decode_speculate and sf_decode_path act as on
 * shafa_hipd_sf_decode.  NULL b, d_in_n, d_tables or d_n_symbols: SHAFA_OUTSIDE_MODULE. */
int shafa_hipd_sf_decode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                             const shafa_code_table *d_tables, const uint64_t *d_n_symbols,
                             uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap);

/* shafa_hipd_rle_decode with the block sizes in DEVICE memory: block b decodes the d_in_n[b] (<= h_in_cap[b]) bytes at
 * d_in + h_in_off[b].  Results equal shafa_hipd_rle_decode with h_in_n = d_in_n; d_in_n[b] > h_in_cap[b] is
 * SHAFA_OUTSIDE_MODULE for block b (d_out_n[b] = 0).  Enqueues only, as shafa_hipd_sf_decode_dev: with it an RLE
 * session decodes host-free (sf_decode_dev's d_n_symbols is this call's d_in_n).  NULL b or d_in_n: SHAFA_OUTSIDE_MODULE;
 * SHAFA_LACK_OF_MEMORY as for shafa_hipd_rle_decode, by h_in_cap. */
int shafa_hipd_rle_decode_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                              const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                              uint8_t *d_out, const uint64_t *h_out_off, const uint64_t *h_out_cap, uint64_t *d_out_n);

/* The decoded sizes of RLE blocks without decoding them: d_out_n[b] = the size shafa_hipd_rle_decode_dev leaves for the same
 * block with h_out_cap[b] = SHAFA_RLE_DECODE_MAX.  The arguments are that entry's without the output buffer; no byte of
 * output is written anywhere, and d_in is only read.  Per-block codes through shafa_hipd_finish, as for every entry:
 *   the stream ends inside a {0, symbol, count} triple, or its output would pass SHAFA_RLE_DECODE_MAX
 *                                          SHAFA_FILE_UNRECOGNIZABLE, d_out_n[b] = 0;
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_out_n[b] = 0 (no byte of the block is read).
 * d_in_n[b] = 0 is size 0 and success.  There is no capacity, so no block is ever SHAFA_LACK_OF_MEMORY.  Every token
 * yields at least one byte: a block with d_in_n[b] > 0 measures 0 only when it was refused.
 * Two launches — every 8 KiB tile on its own, then one workgroup per block — in which no workgroup waits for another; the
 * grid is the tile count of the call, so any nblocks <= max_blocks with any mix of capacities is measured.  The device
 * workspace is 16 bytes per 8 KiB of sum(h_in_cap) plus 20 bytes per block.
 * Enqueues only, as shafa_hipd_rle_decode_dev: d_in_n is never read on the host, no device-to-host copy is issued and nothing
 * is synchronised; the one exception is the batch's growth, from nblocks and h_in_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_in_n, d_out_n,
 * h_in_off or h_in_cap, or an h_in_off[b] that is not a multiple of 16: SHAFA_OUTSIDE_MODULE; nblocks > the batch's
 * max_blocks: SHAFA_LACK_OF_MEMORY (so is a call of 2^31 tiles or more); nblocks <= 0: success. */
int shafa_hipd_rle_decoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n);

/* The RLE sizes of input blocks without encoding them: d_out_n[b] = the size shafa_hipd_rle_encode leaves for the d_in_n[b]
 * (<= h_in_cap[b]) bytes at d_in + h_in_off[b] when it is given room enough (block_compression's size, f.c:29-55).  Per
 * maximal run of byte s with length L that is 3 * (L / 255), plus for m = L % 255: 0 if m == 0; 3 if s == 0 or m >= 4; else m.
 * Runs end at the block's end.  No byte of output is written anywhere except d_out_n[0 .. nblocks) and the batch's error
 * words, and d_in is only read.  Per-block codes through shafa_hipd_finish, as for every entry:
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_out_n[b] = 0 (no byte of the block is read).
 * d_in_n[b] = 0 is size 0 and success.  Any input has an RLE size: no block is ever SHAFA_LACK_OF_MEMORY or
 * SHAFA_FILE_UNRECOGNIZABLE.  With h_out_cap[b] = d_out_n[b], shafa_hipd_rle_encode[_tiles] fills its region exactly.
 * Two launches — every 8 KiB tile on its own, then one workgroup per block — in which no workgroup waits for another; the
 * grid is the tile count of the call, so any nblocks <= max_blocks with any mix of capacities is measured.  The device
 * workspace is 16 bytes per 8 KiB of sum(h_in_cap) plus 20 bytes per block.
 * Enqueues only, as shafa_hipd_rle_decoded_size_dev: d_in_n is never read on the host, no device-to-host copy is issued and
 * nothing is synchronised; the one exception is the batch's growth, from nblocks and h_in_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_in_n, d_out_n,
 * h_in_off or h_in_cap, or an h_in_off[b] that is not a multiple of 16: SHAFA_OUTSIDE_MODULE (a NULL batch comes first);
 * nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY (so is a call of 2^31 tiles or more); nblocks <= 0: success. */
int shafa_hipd_rle_encoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n);

/* The histograms of the blocks' RLE bytes without the RLE bytes: d_freq[b * 256 + s] = the count shafa_hipd_rle_encode leaves
 * in its d_freq for the d_in_n[b] (<= h_in_cap[b]) bytes at d_in + h_in_off[b] when it is given room enough, and d_out_n[b] =
 * the size shafa_hipd_rle_encoded_size_dev leaves, which is the sum of the block's 256 counts.  Per maximal run of byte s with
 * length L, q = L / 255 and m = L % 255 (f.c:29-55): q to each of the counts of 0, s and 255; then, for m > 0, one to each of
 * 0, s and m if s == 0 or m >= 4, else m to s.  Runs end at the block's end; counts that coincide (s == 0, s == 255, s == m)
 * stack.  d_freq[0 .. 256 nblocks) is overwritten, not added to.  No byte of output is written anywhere except d_freq,
 * d_out_n[0 .. nblocks) and the batch's error words, and d_in is only read.  Per-block codes through shafa_hipd_finish:
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_out_n[b] = 0 and 256 zeros (no byte of the block is read).
 * d_in_n[b] = 0 is size 0, 256 zeros and success.  No block is ever SHAFA_LACK_OF_MEMORY or SHAFA_FILE_UNRECOGNIZABLE.
 * With these counts Module T (shafa_hipd_sf_build_codes) and shafa_hipd_sf_encoded_size_dev complete for an RLE file
 * without its .rle bytes.
 * Two launches, as shafa_hipd_rle_encoded_size_dev — every 8 KiB tile on its own (its bytes and the runs inside it, counted
 * in local memory and added to the block's counts with at most 256 atomics per workgroup and block), then one workgroup per
 * block (the runs that touch a tile border: at most two per tile) — in which no workgroup waits for another; the grid is the
 * tile count of the call, so any nblocks <= max_blocks with any mix of capacities is measured.  The device workspace is 16
 * bytes per 8 KiB of sum(h_in_cap) plus 20 bytes per block.
 * Enqueues only, as shafa_hipd_rle_encoded_size_dev: d_in_n is never read on the host, no device-to-host copy is issued and
 * nothing is synchronised; the one exception is the batch's growth, from nblocks and h_in_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_in_n, d_out_n,
 * d_freq, h_in_off or h_in_cap, or an h_in_off[b] that is not a multiple of 16: SHAFA_OUTSIDE_MODULE (a NULL batch comes
 * first); nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY (so is a call of 2^31 tiles or more); nblocks <= 0: success. */
int shafa_hipd_rle_encoded_hist_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_cap, const uint64_t *d_in_n,
                                    uint64_t *d_out_n, uint64_t *d_freq);

/* Where a decoder's output first differs from an original: block b compares the d_a_n[b] (<= h_a_cap[b]) bytes at
 * d_a + h_a_off[b] — a device decoder's output region: d_a and every h_a_off[b] are multiples of 16, the size is device
 * resident — with the h_ref_n[b] bytes at d_ref + h_ref_off[b], which may have ANY byte alignment and lie anywhere in a
 * buffer of any size (64-bit offsets).  With m = min(d_a_n[b], h_ref_n[b]), d_first[b] = the smallest i < m at which the two
 * differ, or m when the first m bytes agree: the blocks are equal iff d_first[b] == d_a_n[b] == h_ref_n[b].  With several
 * differences the first is returned, whatever the scheduling (no atomics).
 * A difference is data, not an error: it sets no error word.  Per-block codes through shafa_hipd_finish:
 *   d_a_n[b] > h_a_cap[b]                  SHAFA_OUTSIDE_MODULE, d_first[b] = 0 (no byte of the block is read).
 * Bytes of a region behind d_a_n[b] (the slack of an exact region is uninitialised) and bytes of ref behind h_ref_n[b] never
 * influence the result.  Neither operand is copied or written.  ref is read in aligned 16-byte words that each hold at least
 * one byte of [ref, ref + h_ref_n[b]), shifted into place; no other byte of it is touched.  Nothing is written except
 * d_first[0 .. nblocks) and the batch's error words.
 * Two launches — every 8 KiB tile on its own, then one workgroup per block — in which no workgroup waits for another; the
 * grid is the tile count of the call.  The device workspace is 16 bytes per 8 KiB of sum(h_a_cap) plus 36 bytes per block.
 * Enqueues only: d_a_n is never read on the host, no device-to-host copy is issued and nothing is synchronised; the one
 * exception is the batch's growth, from nblocks and h_a_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL d_a or d_ref, a d_a
 * that is not a multiple of 16, NULL b, d_a_n, d_first, h_a_off, h_a_cap, h_ref_off or h_ref_n, or an h_a_off[b] that is not
 * a multiple of 16: SHAFA_OUTSIDE_MODULE; nblocks > the batch's max_blocks, or 2^31 tiles or more in sum(h_a_cap):
 * SHAFA_LACK_OF_MEMORY; nblocks <= 0 (with b and the four device pointers given): success. */
int shafa_hipd_compare_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_a, const uint64_t *h_a_off,
                           const uint64_t *h_a_cap, const uint64_t *d_a_n, const uint8_t *d_ref, const uint64_t *h_ref_off,
                           const uint64_t *h_ref_n, uint64_t *d_first);

/* CRC-32 (the zlib / PNG / gzip one: polynomial 0xEDB88320 reflected, init and final XOR 0xFFFFFFFF; the CRC of no byte is 0,
 * of "123456789" 0xCBF43926) of byte regions in device memory: d_crc[b] = the CRC of the d_in_n[b] (<= h_in_cap[b], device
 * resident) bytes at d_in + h_in_off[b].  The offsets are 64-bit and need NO alignment: originals, the segments of a
 * concatenation and decoder regions are digested where they lie.  The region is read as shafa_hipd_compare_dev reads its ref
 * side: in aligned 16-byte words that each hold at least one byte of it, shifted into place; no other byte is touched,
 * nothing is copied, and bytes behind d_in_n[b] (the slack of an exact region, a neighbouring segment) never influence the
 * result.  Nothing is written except d_crc[0 .. nblocks) and the batch's error words.  Per-block codes through
 * shafa_hipd_finish:
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_crc[b] = 0 (no byte of the block is read).
 * Two launches — every 8 KiB tile on its own, then one workgroup per block — in which no workgroup waits for another and
 * no atomic is used: the result does not depend on scheduling.  The device workspace is 16 bytes per 8 KiB of sum(h_in_cap)
 * plus 20 bytes per block.  Enqueues only: d_in_n is never read on the host, no device-to-host copy is issued and nothing is
 * synchronised; the one exception is the batch's growth, from nblocks and h_in_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_in, d_in_n, d_crc,
 * h_in_off or h_in_cap: SHAFA_OUTSIDE_MODULE (a NULL batch comes first); nblocks > the batch's max_blocks, or 2^31 tiles or
 * more in sum(h_in_cap): SHAFA_LACK_OF_MEMORY; nblocks <= 0 (with b, d_in, d_in_n and d_crc given): success. */
int shafa_hipd_crc32_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                         const uint64_t *h_in_cap, const uint64_t *d_in_n, uint32_t *d_crc);

/* The CRC-32 of concatenations, from the parts' finished CRCs and lengths alone (zlib's crc32_combine: crc(A || B) =
 * crc(A) x^(8 |B|) mod P ^ crc(B)).  File f is blocks h_first[f] .. h_first[f] + h_count[f] - 1 of d_crc / d_n, in
 * shafa_hipd_pack_*_files' convention (any blocks, the same block in several files included): d_file_n[f] = the sum of their
 * d_n (64-bit: a file may exceed 4 GiB, a block may have 0 bytes), d_file_crc[f] = the CRC-32 of the bytes they stand for, one
 * after the other.  h_count[f] = 0 is CRC 0 and length 0.  The rule is associative: a call's outputs may be the next call's
 * inputs, which is how groups of blocks digested apart are joined.  No data byte is read.
 * One workgroup per file.  Enqueues only; the device workspace is 8 bytes per file.  No per-block code is set.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_crc, d_n, d_file_crc,
 * d_file_n, h_first or h_count, a negative h_first[f] or h_count[f], or a block range past 2^31 - 1: SHAFA_OUTSIDE_MODULE (a
 * NULL batch or device array comes first); nfiles > the batch's max_blocks: SHAFA_LACK_OF_MEMORY; nfiles <= 0: success. */
int shafa_hipd_crc32_combine_dev(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                                 const uint32_t *d_crc, const uint64_t *d_n, uint32_t *d_file_crc, uint64_t *d_file_n);

/* The positions of a byte pattern (h_pat, pat_n = 1 .. SHAFA_FIND_MAX_PATTERN bytes, on the host) in byte regions in device
 * memory, addressed as shafa_hipd_crc32_dev's: region b is the d_in_n[b] (<= h_in_cap[b], device resident) bytes at
 * d_in + h_in_off[b]; the offsets are 64-bit and need NO alignment, nothing is copied, and bytes behind d_in_n[b] never influence
 * the result.
 * What a match is.  The SHAFA_FIND_NEXT bits of h_flags (NULL = all 0) cut the regions into maximal chains of consecutive
 * regions: region b + 1 continues region b's stream iff h_flags[b] has the bit.  A chain stands for the concatenation of its
 * regions' bytes; empty regions contribute nothing.  A match is every i at which the chain's bytes [i, i + pat_n) equal the
 * pattern; overlapping matches all count ("aaaa" in ten 'a's is 7 matches).  Each match is charged to the region that holds its
 * first byte, at offset o in that region, and is reported as h_pos[b] + o.  Matches charged to a SHAFA_FIND_CONTEXT region are
 * dropped: such a region only supplies bytes to matches that start before it.  Without h_flags every region is its own chain
 * and a match lies wholly inside one region.
 * Outputs.  d_count[b] = the number of matches charged to region b (0 for a context region).  With T = the value of *d_total
 * on the device when the call executes, the call's matches are numbered T, T + 1, ... by region ascending and by offset
 * ascending within a region; match number k is stored at d_hits[k] iff k < max_hits, and *d_total becomes T + sum(d_count).
 * Calls enqueued back to back on one stream with the same d_hits / d_total therefore append (a caller zeroes *d_total once),
 * with no synchronisation in between.  Nothing else is written: d_hits[k] for k >= the new total and for k >= max_hits stays
 * untouched.  d_hits may be NULL iff max_hits == 0 (counts only; no emit launch runs).
 * A match is data and sets no error word.  Per-block codes through shafa_hipd_finish:
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_count[b] = 0; no byte of the block is read and the block
 *                                          counts as empty in its chain.
 * Launches, in none of which a workgroup waits for another or an atomic is used — the result does not depend on scheduling
 * and the same call gives the same d_hits: every 8 KiB tile (numbered from the capacities) counts the matches that lie wholly
 * inside its region; one workgroup per block puts its tiles' counts in order and finds the matches that start in the region's
 * last pat_n - 1 bytes and run into the following regions of the chain (at most 2 (pat_n - 1) bytes, empty regions skipped,
 * up to the first region without SHAFA_FIND_NEXT); one workgroup runs over the blocks' counts; with max_hits > 0 the tiles
 * that hold a match find them again and store them — a tile without one is not read a second time.  A region is read in
 * aligned 16-byte words that each hold at least one byte of it, shifted into place, and in single bytes inside it; no other
 * byte is touched.  The device workspace is at most 16 bytes per 8 KiB of sum(h_in_cap) plus 72 bytes per block plus 512.
 * Enqueues only: d_in_n and *d_total are never read on the host, no device-to-host copy is issued and nothing is synchronised;
 * the one exception is the batch's growth, from nblocks and h_in_cap.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), in this order: NULL b (first),
 * d_in, d_in_n, d_count, d_total or h_pat, pat_n of 0 or above SHAFA_FIND_MAX_PATTERN, NULL d_hits with max_hits > 0:
 * SHAFA_OUTSIDE_MODULE; then nblocks <= 0: success (*d_total is left as it is, the host arrays may be NULL); nblocks > the
 * batch's max_blocks, or 2^31 tiles or more in sum(h_in_cap): SHAFA_LACK_OF_MEMORY; NULL h_in_off, h_in_cap or h_pos, a flag
 * bit other than the two defined, SHAFA_FIND_NEXT on the last region: SHAFA_OUTSIDE_MODULE. */
#define SHAFA_FIND_MAX_PATTERN 256
#define SHAFA_FIND_NEXT 1    /* h_flags[b]: region b + 1 continues region b's stream */
#define SHAFA_FIND_CONTEXT 2 /* h_flags[b]: matches that START in region b are not reported */
int shafa_hipd_find_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                        const uint64_t *h_in_cap, const uint64_t *d_in_n, const uint8_t *h_flags, const uint64_t *h_pos,
                        const uint8_t *h_pat, uint32_t pat_n, uint64_t max_hits, uint64_t *d_hits, uint64_t *d_count,
                        uint64_t *d_total);

/* ---- Byte planes: arrays of typed elements <-> one byte string per byte of the element ------------------------------------
 * The codec is order-0 over bytes; the bytes of a typed element (the sign and exponent byte of a float, its mantissa bytes, the
 * high bytes of small integers) have very different histograms, so each is coded apart.  Block b is d_n[b] (<= h_cap[b],
 * device resident) ELEMENTS of `elem` = 1, 2, 4 or 8 bytes; elem = 1 is a plain copy through the same code.
 *   element side   the block's elem * d_n[b] bytes at d_in (d_out) + h_in_off[b] (h_out_off[b]); the offsets are 64-bit and
 *                  need NO alignment, as shafa_hipd_crc32_dev's: tensors are transposed where they lie.
 *   plane side     plane j of block b = byte j of every element, little-endian (plane 0 is the least significant byte):
 *                  d_n[b] bytes at d_planes + h_plane_off[b * elem + j].  d_planes and every plane offset are multiples of 16
 *                  (the caller allocates this side).
 * shafa_hipd_split_planes_dev reads the element side and writes the planes; shafa_hipd_merge_planes_dev is its inverse.
 * What is read.  split reads the element side in aligned 16-byte words that each hold at least one byte of the region, shifted
 * into place; no other byte is touched, nothing is copied, and bytes outside the region never influence the result.  merge
 * reads a plane in aligned 16-byte words that each hold at least one of its d_n[b] bytes.
 * What is written.  split writes the d_n[b] bytes of each plane and nothing behind them (whole 16-byte words, single bytes
 * in the last one).  merge writes the elem * d_n[b] bytes of the region and nothing else: aligned 16-byte words that lie
 * wholly inside it, single bytes at its two ends; the up to 15 bytes on either side of an unaligned region are untouched.
 * Per-block codes through shafa_hipd_finish:
 *   d_n[b] > h_cap[b]                      SHAFA_OUTSIDE_MODULE; no byte of the block is read or written, other blocks are
 *                                          unaffected.
 * One launch for all blocks, in which no workgroup waits for another: tiles of SHAFA_PLANES_TILE elements, numbered from the
 * capacities, a lane transposing 16 elements at a time in registers (elem words of the element side, one word of each plane:
 * per plane a wave's stores are 1 KiB contiguous); a tile at or behind d_n[b] exits.  The only atomic is the error word above.
 * The device workspace is (20 + 8 elem) bytes per block plus 20.  Enqueues only: d_n is never read on the host, no
 * device-to-host copy is issued and nothing is synchronised; the one exception is the batch's growth, from nblocks.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), in this order: NULL b (first),
 * d_in / d_out, d_planes or d_n, an elem other than 1, 2, 4, 8: SHAFA_OUTSIDE_MODULE; then nblocks <= 0: success (the host
 * arrays may be NULL); nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY; NULL h_cap: SHAFA_OUTSIDE_MODULE; an
 * elem * h_cap[b] or their sum past 64 bits, or 2^31 tiles or more in the capacities: SHAFA_LACK_OF_MEMORY; NULL h_in_off /
 * h_out_off or h_plane_off, a d_planes or an h_plane_off[b * elem + j] that is no multiple of 16: SHAFA_OUTSIDE_MODULE. */
#define SHAFA_PLANES_TILE 8192 /* elements */
int shafa_hipd_split_planes_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                const uint64_t *h_plane_off);
int shafa_hipd_merge_planes_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                const uint64_t *h_out_off);

/* ---- Byte planes of deltas: the same transposes with every element XORed with the element of a base ------------------------
 * A checkpoint follows a checkpoint and a fine-tune its base model: against such a base most elements are bit-identical and
 * the others share their high bytes, so the planes of (element XOR base element) are long runs of zero — what RLE and the
 * Shannon-Fano coder behind it shrink most.  The XOR is done inside the transposes, which touch every element once anyway: no
 * temporary, 3 bytes of traffic per tensor byte in either direction.
 * shafa_hipd_split_planes_xor_dev: plane j of block b = byte j of (element XOR base element).
 * shafa_hipd_merge_planes_xor_dev: its inverse, element = (the element put together from the planes) XOR base element.
 * Everything said above of the plain entries holds: the blocks, the element side, the plane side, the capacities, what is
 * written (exactly what the plain entries write), the per-block code, one launch in which no workgroup waits for another.
 *   base side      block b's base is elem * d_n[b] bytes at d_base + h_base_off[b]; the offsets are 64-bit and need NO
 *                  alignment, and a base's alignment is independent of its element side's.  h_base_off[b] ==
 *                  SHAFA_PLANES_NO_BASE: the block has none; its result is the plain entry's byte for byte and no byte is
 *                  read through d_base for it, so one launch takes new tensors and changed ones together.
 * What is read.  The base side is read the way split reads its element side: aligned 16-byte words that each hold at least
 * one byte of the region, shifted into place; bytes outside the region never influence a result.  Every base element is read
 * once (merge into an unaligned region reads 16 base bytes a wave twice, as it does 16 bytes of each plane).  A pass of split
 * in which both the element side and the base are 16-aligned takes its coalesced path, as in the plain entry.
 * No overlap.  The base regions must not overlap what the call writes: the planes for split, the output regions for merge.
 * Into an unaligned output a lane stores the word that holds the tail of its neighbour's unit, which the neighbour may not
 * have read from the base yet: merging in place (d_out the base) is NOT supported.
 * Per-block codes through shafa_hipd_finish:
 *   d_n[b] > h_cap[b]                      SHAFA_OUTSIDE_MODULE; no byte of the block, its base included, is read or written.
 * The device workspace is (28 + 8 elem) bytes per block plus 20: the plain entries' and 8 bytes per block for the base
 * offsets.  Enqueues only, as the plain entries.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), in the plain entries' order:
 * NULL b (first), d_in / d_out, d_planes, d_n or d_base, an elem other than 1, 2, 4, 8: SHAFA_OUTSIDE_MODULE; then
 * nblocks <= 0: success; nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY; NULL h_cap: SHAFA_OUTSIDE_MODULE; the
 * capacities' bounds: SHAFA_LACK_OF_MEMORY; NULL h_in_off / h_out_off, h_plane_off or h_base_off, a d_planes or a plane
 * offset that is no multiple of 16: SHAFA_OUTSIDE_MODULE. */
#define SHAFA_PLANES_NO_BASE UINT64_MAX /* h_base_off[b]: block b has no base */
int shafa_hipd_split_planes_xor_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                    const uint64_t *h_in_off, const uint8_t *d_base, const uint64_t *h_base_off,
                                    const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes, const uint64_t *h_plane_off);
int shafa_hipd_merge_planes_xor_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                    const uint64_t *h_plane_off, const uint8_t *d_base, const uint64_t *h_base_off,
                                    const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off);

/* ---- Byte planes of differences: the same transposes of every element's difference to the element in front ------------------
 * Data that runs along the element axis — document offsets, position ids, sorted ids and COO / CSR indices, timestamps, sampled
 * signals — has a low byte that walks through all 256 values even where every step is + 1, and an order-0 coder gains nothing
 * from it; the difference to the element in front is small, and its planes are what RLE and Shannon-Fano shrink.  The
 * transform, with M = 2^(8 elem) and x[i] element i of the block read as an unsigned little-endian integer (the bit pattern,
 * whatever the dtype), x[-1] = 0 — every block starts afresh:
 *   d[i] = (x[i] - x[i-1]) mod M
 *   z[i] = ((d[i] << 1) mod M) XOR (M - 1 if d[i] >= M / 2, else 0)      the zigzag fold: small differences of either sign
 *                                                                         become small z
 *   plane j of the block = byte j of z[i]
 * and back:
 *   d[i] = (z[i] >> 1) XOR (M - 1 if z[i] is odd, else 0)
 *   x[i] = (x[i-1] + d[i]) mod M
 * It is a bijection on any input: random bit patterns come back bit for bit.
 * shafa_hipd_split_planes_diff_dev writes the planes of z; shafa_hipd_merge_planes_diff_dev is its inverse.
 * Everything said above of the plain entries holds, with their arguments in their order: the blocks, the element side at ANY
 * alignment, the plane side at multiples of 16, elem = 1, 2, 4 or 8, the capacities on the host and the sizes device resident,
 * what is written — exactly the plain entries' bytes: merge leaves the up to 15 bytes on either side of an unaligned region
 * untouched, split writes nothing behind a plane's d_n[b] bytes — and the per-block code:
 *   d_n[b] > h_cap[b]                      SHAFA_OUTSIDE_MODULE; no byte of the block is read or written, other blocks are
 *                                          unaffected.
 * What is read.  split reads what the plain split reads and, one lane a wave, the element in front of the wave's first unit
 * (elem single bytes inside the region): 2 bytes of traffic per tensor byte.  merge reads the planes TWICE, in the plain merge's
 * aligned words: 3 bytes of traffic per tensor byte.
 * Launches.  split is one launch, the plain split's with the subtraction and the fold in front of the transposition.  merge is
 * three on the stream: the sum of the d's of every tile of SHAFA_PLANES_TILE elements (a tile at or behind d_n[b] is not read),
 * one workgroup a block that turns the sums of the block's tiles into exclusive prefixes, and the plain merge with a prefix
 * sum over the tile in element order on top of the tile's prefix.  In none of them does a workgroup wait for another: no
 * tickets, no look-back, no flags.
 * The device workspace is the plain entries', (20 + 8 elem) bytes per block plus 20, and for merge 8 bytes more per tile of the
 * capacities; one that cannot be had is SHAFA_LACK_OF_MEMORY.  Enqueues only, as the plain entries.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), the plain entries' in the plain
 * entries' order. */
int shafa_hipd_split_planes_diff_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_in,
                                     const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                     const uint64_t *h_plane_off);
int shafa_hipd_merge_planes_diff_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint8_t *d_planes,
                                     const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                     const uint64_t *h_out_off);

/* ---- Byte planes of lagged differences: the difference to the element h_lag[b] in front ------------------------------------
 * Data that runs along an axis is seldom stored along it: a [T, C] sensor log runs along T with the channels interleaved, an
 * [H, W, 3] image along W at distance 3 and along H at distance 3 W, a [steps, params] stack of checkpoints along steps.  The
 * difference to the flat neighbour subtracts one channel from another; the difference to the element one axis stride in front
 * is the small one.  With M = 2^(8 elem), x[i] element i of the block as an unsigned little-endian integer, L = h_lag[b] >= 1
 * (a host array with ONE LAG PER BLOCK, so one launch per element size serves any mix of shapes) and x[i] = 0 for i < 0 —
 * every block starts afresh:
 *   d[i] = (x[i] - x[i-L]) mod M,   z[i] = the zigzag fold of d[i] (above),   plane j of the block = byte j of z[i]
 * and back: d[i] unfolded, x[i] = (x[i-L] + d[i]) mod M — the block seen as rows of L columns, a prefix sum down every column.
 * It is a bijection on any input.  With L >= d_n[b] the planes are those of the fold of x itself; any L up to 2^64 - 1 is
 * legal.  With L = 1 both entries produce byte for byte what the _diff_dev entries produce.
 * shafa_hipd_split_planes_lag_dev writes the planes of z; shafa_hipd_merge_planes_lag_dev is its inverse.
 * Everything said above of the plain entries holds — the blocks, the plane side at multiples of 16, elem = 1, 2, 4 or 8, the
 * capacities on the host and the sizes device resident, what is written: exactly the plain entries' bytes and nothing outside
 * them, the per-block code (d_n[b] > h_cap[b]: SHAFA_OUTSIDE_MODULE, no byte of the block read or written) — with ONE
 * exception, which is deliberate:
 *   element side   d_in / d_out and every h_in_off[b] / h_out_off[b] are MULTIPLES OF elem.  A tensor's elements always lie at
 *                  multiples of their size; bytes at odd addresses are what the record entries are for.
 * Launches.  split is one launch: the plain split's units, each with the unit L elements in front of it read from the block's
 * own region as a base (mostly from L2 where L is small): 2 bytes of traffic per tensor byte.  merge is up to three on the
 * stream.  A block is cut into chunks of G rows by strips of W columns, one column a lane:
 *   L >= SHAFA_PLANES_LAG_STRIP   W = SHAFA_PLANES_LAG_STRIP, S = 1
 *   L <  SHAFA_PLANES_LAG_STRIP   W = L, and the workgroup's lanes are S = SHAFA_PLANES_LAG_STRIP / L (rounded down) segments of
 *                                 rows, so a round of rows is a contiguous run of the block
 *   G = SHAFA_PLANES_LAG_ROWS * S * m, m = max(1, items / SHAFA_PLANES_LAG_ITEMS rounded down), items = the chunk-strips that
 *   h_cap[b] would have at m = 1
 * all from h_cap[b] and h_lag[b], which the host has.  Launch 1 writes the column sums (mod M, elem bytes each) of every chunk
 * that has a chunk behind it, launch 2 turns them into exclusive prefixes down each column, launch 3 rebuilds the elements
 * chunk by chunk on top of its prefix (in a strip of SHAFA_PLANES_LAG_STRIP columns a lane takes four columns next to each
 * other and a quarter of the rows, so the planes are read a dword and the elements written four at a time); where no block
 * of the call has more than one chunk, launches 1 and 2 are not made.  No workgroup ever waits for another: no tickets, no
 * look-back, no flags; the only atomic is the error word.  The planes are read twice: 3 bytes of traffic per tensor byte.
 * The device workspace is (28 + 8 elem) bytes per block plus 20 and, for a merge with a block of more than one chunk,
 * elem * SHAFA_PLANES_TILE / 8 bytes per tile of the capacities: at most 1/8 of the capacities' bytes plus elem KiB per block.
 * One that cannot be had is SHAFA_LACK_OF_MEMORY.  Enqueues only, as the plain entries.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), the plain entries' in the plain
 * entries' order, and with the host arrays (behind the plane offsets' alignment), each SHAFA_OUTSIDE_MODULE: NULL h_lag or an
 * h_lag[b] of 0; a d_in / d_out or an h_in_off[b] / h_out_off[b] that is no multiple of elem. */
#define SHAFA_PLANES_LAG_STRIP 256  /* columns of a strip; below it a block's rows are taken whole */
#define SHAFA_PLANES_LAG_ROWS 32    /* rows a lane takes at a time */
#define SHAFA_PLANES_LAG_ITEMS 4096 /* chunk-strips of a block beyond which its chunks grow */
int shafa_hipd_split_planes_lag_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint64_t *h_lag,
                                    const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n,
                                    uint8_t *d_planes, const uint64_t *h_plane_off);
int shafa_hipd_merge_planes_lag_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint64_t *h_lag,
                                    const uint8_t *d_planes, const uint64_t *h_plane_off, const uint64_t *h_cap,
                                    const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off);

/* ---- Byte planes of Lorenzo differences: the differences along up to three lags at once -----------------------------------
 * Data that is smooth along SEVERAL axes — a 2-D or 3-D simulation field, a stack of images, [step, y, x] snapshots — keeps most
 * of its redundancy when only one axis is differenced.  The integer Lorenzo predictor of the scientific-data codecs differences
 * along every axis in turn, on the bit patterns.  Block b has nlags (1 .. SHAFA_PLANES_GRID_LAGS, one number for the call) slots
 * h_lags[b * nlags + k]: the first is >= 1, every further slot is 0 (unused, and then so is every slot behind it) or greater
 * than the slot in front of it, so one launch per element size serves any mix of 1-D, 2-D and 3-D tensors.  With M = 2^(8 elem),
 * x the block's elements as unsigned little-endian integers, x[i] = 0 for i < 0, (S^L x)[i] = x[i - L] and L1 < L2 < L3 the
 * used lags:
 *   d = (1 - S^L1)(1 - S^L2)(1 - S^L3) x mod M,  i.e.  d[i] = sum over the subsets A of the used lags of (-1)^|A| x[i - sum A]
 *   z[i] = the zigzag fold of d[i] (above),   plane j of the block = byte j of z[i]
 * and back: d unfolded, then x[i] += x[i - L] in place once per lag, in any order (the passes commute).  It is a bijection on any
 * input.  The difference does not start afresh at the end of a row or a slab — a row's first element is taken against the last
 * one of the row in front — which is what makes the transform a product of flat lags.  A lag at or past h_cap[b] subtracts
 * nothing.  It does not always pay: every further difference doubles the variance of whatever noise the data carries.
 * shafa_hipd_split_planes_grid_dev writes the planes of z; shafa_hipd_merge_planes_grid_dev is its inverse.  With nlags = 1
 * both write byte for byte what the _lag_dev entries write, with a block's lags (1, 0, 0) what the _diff_dev entries write.
 * Everything said of the _lag_dev entries holds: the element side at multiples of elem, the plane side at multiples of 16, the
 * capacities on the host and the sizes device resident, exactly the plain entries' bytes written and nothing outside them, the
 * per-block code (d_n[b] > h_cap[b]: SHAFA_OUTSIDE_MODULE, no byte of the block read or written in any of the launches).
 * Launches.  split is one launch: the _lag_dev split with one base unit per non-empty subset of the block's lags (up to seven),
 * read at the summed distance and subtracted or added, one at a time: 2 bytes of HBM traffic per tensor byte while the taps
 * hit L2.  merge is a chain on the stream in which no workgroup waits for another: a first pass from the planes to the elements
 * at the block's smallest lag — the _diff_dev merge's three launches for the blocks where that lag is 1, the _lag_dev merge's up
 * to three for the others, each family skipping the other's blocks — then, per further lag, the _lag_dev merge's launches with
 * the elements themselves as their source, in place (no planes, no unfold; blocks without that lag are skipped).  3 bytes of
 * traffic per tensor byte for the first pass and at most 3 for each further one.  The device workspace is the _lag_dev merge's
 * with (44 + 8 elem) bytes per block, three lags where it has one: one region of sums, which the passes use in turn.  One that cannot be had is
 * SHAFA_LACK_OF_MEMORY.  Enqueues only.
 * Argument errors return with nothing enqueued (checked before HIP is touched): the _lag_dev entries' in their order; an nlags
 * outside 1 .. SHAFA_PLANES_GRID_LAGS with elem; and where those entries check their lags, each SHAFA_OUTSIDE_MODULE: NULL
 * h_lags, a first slot of 0, a slot not greater than a non-zero slot in front of it, a non-zero slot behind a 0. */
#define SHAFA_PLANES_GRID_LAGS 3
int shafa_hipd_split_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                     const uint64_t *h_lags, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                                     const uint64_t *d_n, uint8_t *d_planes, const uint64_t *h_plane_off);
int shafa_hipd_merge_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                     const uint64_t *h_lags, const uint8_t *d_planes, const uint64_t *h_plane_off,
                                     const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out, const uint64_t *h_out_off);

/* ---- Plane histograms of Lorenzo differences: which lags pay, without the planes ------------------------------------------
 * Whether a tensor compresses best as plain planes, along one axis or along several is a property of its data.  Each candidate's
 * size follows from the histograms of its planes (shafa_hipd_sf_build_codes, shafa_hipd_sf_encoded_size_dev), and the histograms
 * need no planes: this entry reads the elements and leaves the counts.
 *   d_freq[(b * elem + j) * 256 + s] = the number of elements i < d_n[b] of block b whose byte j of z[i] is s,
 * z exactly what shafa_hipd_split_planes_grid_dev writes for the block's row of lags.  One addition to those entries' rule for a
 * row: a row of all zeros is the PLAIN candidate, z = x, no difference and no fold — the counts of shafa_hipd_split_planes_dev's
 * planes.  (A first slot of 0 with a non-zero slot behind it stays SHAFA_OUTSIDE_MODULE; a lag at or past h_cap[b] subtracts
 * nothing, as there.)  Each plane's 256 counts sum to d_n[b].  The layout is shafa_hipd_hist256's with nblocks * elem
 * histograms: shafa_hipd_sf_build_codes and shafa_hipd_sf_encoded_size_dev take it as it is.  The call zeroes its nblocks * elem *
 * 256 counts itself and writes nothing else.
 * Blocks are only read and MAY OVERLAP OR COINCIDE on the element side: one tensor, one block per candidate row of lags, is the
 * use.  The element side lies at multiples of elem (1, 2, 4 or 8), as the _grid_dev entries'; there is no plane side.
 * Per-block code through shafa_hipd_finish: d_n[b] > h_cap[b] is SHAFA_OUTSIDE_MODULE, no byte of the block is read and its
 * counts are 0.
 * Launches.  One memset and one launch, enqueued only; no workgroup waits for another.  A workgroup walks a run of
 * SHAFA_PLANES_HIST_RUN consecutive tiles of SHAFA_PLANES_TILE elements (numbered from the capacities), counts into 16 or 32
 * KiB of LDS — 32, 8, 8 or 4 replicas of the elem histograms, 32-bit bins, which a run cannot overflow — and adds its non-zero bins to the
 * block's counts with 64-bit global atomics when the walk enters another block and at its end.  1 byte of HBM traffic per tensor
 * byte and candidate at the most; candidates on one region that fits the cache read it from there.
 * Argument errors return with nothing enqueued (checked before HIP is touched), in the _grid_dev split's order with d_freq in
 * d_planes' place and no plane-side rule: NULL b, d_in, d_freq or d_n, an nlags outside 1 .. SHAFA_PLANES_GRID_LAGS, an elem
 * other than 1, 2, 4, 8: SHAFA_OUTSIDE_MODULE; nblocks <= 0: SHAFA_SUCCESS; nblocks past the batch's: SHAFA_LACK_OF_MEMORY;
 * NULL h_cap: SHAFA_OUTSIDE_MODULE; capacities whose bytes pass 64 bits or whose tiles number 2^31 or more:
 * SHAFA_LACK_OF_MEMORY; NULL h_in_off or h_lags, d_in or an offset off a multiple of elem, a malformed row:
 * SHAFA_OUTSIDE_MODULE. */
#define SHAFA_PLANES_HIST_RUN 8 /* tiles a workgroup counts before it adds its bins to the block's counts */
int shafa_hipd_hist_planes_grid_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                    const uint64_t *h_lags, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                                    const uint64_t *d_n, uint64_t *d_freq);

/* ---- Error-bounded fields: quantise inside the Lorenzo split, restore behind the merge -------------------------------------
 * The fields the _grid_dev entries are for are nearly always float or double, and the Lorenzo differences of raw float bit
 * patterns leave every mantissa byte raw.  The codecs the predictor was taken from (SZ, cuSZ) quantise each value under an error
 * bound first and difference the integers exactly.  These entries are the _grid_dev pair with that quantiser in the split and the
 * restorer behind the merge; no temporary of codes exists.  T is float at elem 4 and double at elem 8 (any other elem:
 * SHAFA_OUTSIDE_MODULE).  Block b has two host doubles, h_step[b] and h_bound[b], both exactly representable in T, finite, normal
 * and > 0; inv = T(1.0 / step), the double division rounded to T once, is finite and not 0.  Every operation below is ONE IEEE
 * operation in T, rounded to nearest even, none contracted into an FMA:
 *   t    = x * inv
 *   in   = |t| < 2^(8 elem - 2)                       (false for a NaN)
 *   code = (signed integer of 8 elem bits) (in ? rint(t) : 0)
 *   x'   = T(code) * step                             (from the INTEGER: a rint of -0.0 restores as +0.0)
 *   good = in and (elem 4: |double(x) - double(x')| <= double(bound), the subtraction in double;
 *                  elem 8: |x - x'| <= bound, the rounded subtraction)
 * The planes are those shafa_hipd_split_planes_grid_dev writes for the block's lags over the array of codes taken as unsigned
 * integers, byte for byte; a position in front of the block is the bit pattern 0, whose code is 0.  An element that is not good
 * is an OUTLIER — a NaN, an infinity, a value past the code range or one whose restored value misses the bound: its code still
 * goes into the planes, and it is recorded as well.  The merge restores every element as x' and then stores the outliers' own
 * bits on top: an outlier comes back bit for bit, every other element within h_bound[b] (-0.0 may come back as +0.0).  The
 * guarantee is checked per element on the device, against the very x' the merge will make.  step and bound are apart on
 * purpose: with step = 2 bound the rounding of x' throws elements near a tie over the bound; a step a little below 2 bound keeps
 * them inside.
 * Outlier records.  A record is 16 bytes, {u64 position in the block, u64 the element's bits in the low 8 elem bits}.  Block b's
 * records start at record h_outl_off[b] of d_outl and number at most h_outl_cap[b] (0 is legal).  The split zeroes
 * d_outl_n[0 .. nblocks) itself; a lane with an outlier takes a slot with a 64-bit atomic add on d_outl_n[b] and writes the record
 * only where slot < capacity.  After shafa_hipd_finish d_outl_n[b] is the number of outliers FOUND: a count above the capacity is
 * the signal, not an error; the planes are complete either way and nothing is written past a block's capacity.  The order of the
 * records within a block is not defined.
 * Everything the _grid_dev pair says of the blocks, the lags, both sides' alignment, the capacities and d_n holds here, what is
 * written and the per-block code for d_n[b] > h_cap[b] included.
 * Launches.  split: a memset of d_outl_n and ONE launch, the grid split's with every loaded unit of 16 elements — the lane's own
 * and every tap's — quantised in registers before it is subtracted or added.  merge: the _grid_dev merge's chain as it is, then
 * a restore pass in place over the elements (code -> T(code) * step) and a patch pass, one thread per record of h_outl_n[b],
 * which stores the record's bits at its position; a position >= d_n[b] gives the block SHAFA_OUTSIDE_MODULE and nothing is
 * written for that record.  The patch pass is not enqueued where the call has no records.  No workgroup waits for another.
 * Enqueues only.
 * Argument errors return with nothing enqueued (checked before HIP is touched): the _grid_dev entries' in their order, and where
 * those check their lags, each SHAFA_OUTSIDE_MODULE: NULL h_step or h_bound; a step or bound that is not finite, not normal, not
 * > 0 or not exactly representable in T, or an inv that is 0 or not finite; NULL d_outl_n, h_outl_off or h_outl_cap (h_outl_n);
 * NULL d_outl while any capacity (count) is not 0. */
int shafa_hipd_split_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const double *h_step, const double *h_bound,
                                           const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n,
                                           uint8_t *d_planes, const uint64_t *h_plane_off, uint64_t *d_outl,
                                           const uint64_t *h_outl_off, const uint64_t *h_outl_cap, uint64_t *d_outl_n);
int shafa_hipd_merge_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const double *h_step, const uint8_t *d_planes,
                                           const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n,
                                           const uint64_t *d_outl, const uint64_t *h_outl_off, const uint64_t *h_outl_n,
                                           uint8_t *d_out, const uint64_t *h_out_off);

/* ---- Field sizes under an error bound: the quantising split's plane histograms, without the planes -------------------------
 * Which lags to take under a bound, how large a field comes out at a given bound, which bound fits a budget: each follows from
 * the histograms of the planes shafa_hipd_split_planes_grid_quant_dev would write and from the number of its outliers, and
 * neither needs a plane or a record.  This entry is shafa_hipd_hist_planes_grid_dev over the CODES:
 *   d_freq[(b * elem + j) * 256 + s] = the number of elements i < d_n[b] of block b whose byte j of z[i] is s,
 * z exactly what shafa_hipd_split_planes_grid_quant_dev writes for the block's row of lags, h_step[b] and h_bound[b] — the codes
 * of "Error-bounded fields" above, their Lorenzo differences, the zigzag fold.  The layout is shafa_hipd_hist256's with nblocks *
 * elem histograms, which shafa_hipd_sf_build_codes and shafa_hipd_sf_encoded_size_dev take as it is; each plane's 256 counts sum
 * to d_n[b].
 *   d_outl_n[b] = the number of elements i < d_n[b] of block b that are not good by that section's rule,
 * the number the split leaves in its own d_outl_n[b].  No record is written and there is no capacity.  The call zeroes its
 * nblocks * elem * 256 counts and d_outl_n[0 .. nblocks) itself and writes nothing else.
 * elem is 4 or 8 (T float or double).  A row of lags follows the _grid_quant_dev split's rule: the first slot >= 1, the others 0
 * or increasing.  There is NO plain candidate here, a row of zeros is malformed: the split cannot make that item.  h_step and
 * h_bound as the split takes them.
 * Blocks are only read and MAY OVERLAP OR COINCIDE on the element side, which lies at multiples of elem: one tensor, one block
 * per (row of lags, step), is the use.
 * Per-block code through shafa_hipd_finish: d_n[b] > h_cap[b] is SHAFA_OUTSIDE_MODULE, no byte of the block is read and its
 * counts are 0.
 * Launches.  Two memsets and one launch, enqueued only; no workgroup waits for another.  The walk, the LDS bins and the 64-bit
 * global atomics are shafa_hipd_hist_planes_grid_dev's.  A lane counts its outliers in a register; where a workgroup adds its
 * bins to block b's counts, each of its waves that found an outlier adds its sum to d_outl_n[b] with one 64-bit atomic — a
 * tensor in which every element is an outlier costs no more atomics than a clean one has non-zero bins.
 * Argument errors return with nothing enqueued (checked before HIP is touched), in shafa_hipd_hist_planes_grid_dev's order: NULL
 * b, d_in, d_freq or d_n, an nlags outside 1 .. SHAFA_PLANES_GRID_LAGS, an elem other than 4, 8: SHAFA_OUTSIDE_MODULE; nblocks
 * <= 0: SHAFA_SUCCESS; nblocks past the batch's: SHAFA_LACK_OF_MEMORY; NULL h_cap: SHAFA_OUTSIDE_MODULE; capacities whose bytes
 * pass 64 bits or whose tiles number 2^31 or more: SHAFA_LACK_OF_MEMORY; NULL h_in_off or h_lags, d_in or an offset off a
 * multiple of elem, a malformed row; then NULL h_step or h_bound, a step, bound or inv the split refuses, NULL d_outl_n:
 * SHAFA_OUTSIDE_MODULE. */
int shafa_hipd_hist_planes_grid_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                          const uint64_t *h_lags, const double *h_step, const double *h_bound, const uint8_t *d_in,
                                          const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_freq,
                                          uint64_t *d_outl_n);

/* ---- Point-wise relative bounds: mantissas rounded to the kept bits, in integer arithmetic --------------------------------
 * One absolute bound serves a field whose values are all of one size.  A field that spans decades, and the bfloat16 and float16
 * tensors torch users hold, want "keep k mantissa bits" instead: |x - x'| <= 2^-(keep + 1) |x| for every normal element.  These
 * three entries are the _grid_quant_dev split and merge and the _grid_quant_dev histogram with that quantiser for rint(x / step):
 * the mantissa rounded to `keep` bits, half to even, the carry free to enter the exponent ("bit rounding").  It is integer work
 * on the element's own bits, so the rule is exact and needs no slack.  elem is 2, 4 or 8 (any other: SHAFA_OUTSIDE_MODULE).
 * Block b has two host uint32_t, h_mant[b], the format's mantissa width — 7 (bfloat16) or 10 (float16) at elem 2, 23 at elem 4,
 * 52 at elem 8; one call may mix the two 16-bit formats — and h_keep[b] <= h_mant[b], the mantissa bits kept.
 * With W = 8 elem and d = mant - keep, in unsigned W-bit integer arithmetic on the element's bits x:
 *   S    = x >> (W-1)                      M = x & (2^(W-1) - 1)
 *   INF  = (2^(W-1-mant) - 1) << mant      MIN = 1 << mant
 *   R    = M >= INF ? M >> d                                        (Inf / NaN: truncated, never carried)
 *        : d == 0   ? M
 *        :            (M + (2^(d-1) - 1) + ((M >> d) & 1)) >> d     (half to even; the carry may enter the exponent)
 *   code = S ? -R : R                      as a signed W-bit integer
 *   M'   = (|code| << d) mod 2^(W-1)       x' = (code < 0) << (W-1) | M'          (what the merge makes of ANY code)
 *   good = (M < MIN or M >= INF) ? M' == M : M' < INF
 * The planes are those shafa_hipd_split_planes_grid_dev writes for the block's lags over the array of codes taken as unsigned
 * W-bit integers, byte for byte, tails included; a position in front of the block is the bit pattern 0, whose code is 0.  An
 * element that is not good is an OUTLIER — a normal value that rounds up to Inf, a denormal with a dropped bit set, a NaN whose
 * payload reaches into the dropped bits (one that would truncate to Inf among them): its code still goes into the planes, and it
 * is recorded under the record contract of "Error-bounded fields" above, word for word (h_outl_off, h_outl_cap, d_outl, d_outl_n
 * zeroed by the call, the slot taken with a 64-bit atomic, written only where slot < capacity, found > capacity the signal).
 * Guarantee, exact: a good normal element comes back with |x - x'| <= 2^-(keep + 1) |x| in real numbers; +-Inf, a good NaN, a
 * good denormal and +0.0 bit for bit; -0.0 as +0.0; an outlier bit for bit.  keep = mant changes nothing but -0.0.
 * A row of lags follows the _grid_quant_dev split's rule.  "No differences" needs no rule of its own: a lag at or past the
 * block's capacity subtracts nothing in split and merge alike.
 * Launches.  split: a memset of d_outl_n and ONE launch, the grid split's with every loaded unit of 16 elements — the lane's own
 * and every tap's — rounded in registers; at elem 2 each half of a word is rounded on its own, no carry passes between them.
 * merge: the _grid_dev merge's chain as it is, a restore pass in place (code -> x') and the patch pass of "Error-bounded fields"
 * where the call has a record.  hist: d_freq and d_outl_n as shafa_hipd_hist_planes_grid_quant_dev leaves them, over these codes:
 * two memsets and one launch.  Blocks of the hist entry are only read and may overlap or coincide.  No workgroup waits for
 * another.  Enqueues only.  Per-block codes through shafa_hipd_finish are the _quant_dev entries', the patch pass's position >=
 * d_n[b] included.
 * Argument errors return with nothing enqueued (checked before HIP is touched): the corresponding _quant_dev entry's in its
 * order, with elem in {2, 4, 8} at the elem check; where that entry checks its steps and bounds, each SHAFA_OUTSIDE_MODULE: NULL
 * h_mant or h_keep, a mant that is not the format's for elem, keep > mant; then the record arguments as there. */
int shafa_hipd_split_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep,
                                           const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n,
                                           uint8_t *d_planes, const uint64_t *h_plane_off, uint64_t *d_outl,
                                           const uint64_t *h_outl_off, const uint64_t *h_outl_cap, uint64_t *d_outl_n);
int shafa_hipd_merge_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                           const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep,
                                           const uint8_t *d_planes, const uint64_t *h_plane_off, const uint64_t *h_cap,
                                           const uint64_t *d_n, const uint64_t *d_outl, const uint64_t *h_outl_off,
                                           const uint64_t *h_outl_n, uint8_t *d_out, const uint64_t *h_out_off);
int shafa_hipd_hist_planes_grid_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, uint32_t nlags,
                                          const uint64_t *h_lags, const uint32_t *h_mant, const uint32_t *h_keep, const uint8_t *d_in,
                                          const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint64_t *d_freq,
                                          uint64_t *d_outl_n);

/* ---- Error statistics: what a bound costs --------------------------------------------------------------------------------
 * The entries above give the rate half of a rate-distortion curve; these three give the distortion half, in one read of the
 * tensor and without a temporary.  All three write one record of SHAFA_ERR_WORDS uint64_t per block, at d_stat + 12 b.  In block
 * b, for element i < d_n[b]: x is the original element, y the element it comes back as, D(.) the conversion to double (exact for
 * bfloat16, float16 and float), the element is FINITE when x and y both are, and e = |D(x) - D(y)| is one double subtraction
 * (exact at elem 2 and 4, the rounded one at elem 8).  Every product and sum is one IEEE double operation, none contracted;
 * overflow to Inf is carried as IEEE carries it.
 *   word 0       n, the d_n[b] the kernel compared
 *   word 1       the finite elements
 *   word 2       the others (x or y is NaN or +-Inf)
 *   word 3       of word 2, those where the bits of y differ from the bits of x
 *   word 4       the outliers: the elements that are not good by the entry's rule; 0 from shafa_hipd_error_dev
 *   word 5       the finite elements with e > h_abs[b] + h_rel[b] |D(x)| (one multiplication, one addition, one comparison);
 *                0 from the other two entries
 *   word 6       the sum of e e over the finite elements, the bits of a double
 *   word 7       the sum of D(x) D(x) over the finite elements, the bits of a double
 *   word 8       the largest e of the finite elements, the bits of a double; 0.0 where there is none
 *   word 9       the smallest i among the finite elements whose e is word 8; 2^64 - 1 where there is none
 *   word 10, 11  the smallest and the largest D(x) of the finite elements, the bits of doubles, a zero extreme as +0.0; +Inf and
 *                -Inf where there is none
 * shafa_hipd_error_dev: y is the element of d_a — a decoder's or a merge's output region: d_a and every h_a_off[b] are multiples
 * of 16, as shafa_hipd_compare_dev has them — and x the element of d_ref at d_ref + h_ref_off[b], any multiple of elem: the
 * original is read where it lies.  elem is 2, 4 or 8; h_cap[b] is block b's capacity in ELEMENTS; h_mant[b] is the format's mantissa
 * width as the _round_dev entries take it (it tells bfloat16 from float16; one call may mix them); h_abs[b] is a double >= 0 or
 * +Inf, h_rel[b] a finite double >= 0.
 * shafa_hipd_error_quant_dev (elem 4 or 8): y is what shafa_hipd_merge_planes_grid_quant_dev gives back for h_step[b] and
 * h_bound[b]: x' where the element is good, x bit for bit where it is an outlier.  There are no lags: a code depends on the
 * element's own bits alone.  shafa_hipd_error_round_dev (elem 2, 4 or 8): the same under the rounding rule of "Point-wise relative
 * bounds" for h_mant[b] and h_keep[b].  The blocks of all three are only read; those of the last two may overlap or coincide: one
 * tensor, one block per bound or per keep, is the use.
 * The sums are taken in a fixed order — a lane's elements by index, a fixed tree across the wave, the waves in order, one partial
 * per tile of SHAFA_PLANES_TILE elements; then a block's partials in ascending order by the same tree — and there are no
 * floating-point atomics: a block's record is a function of its elements, its count and its parameters alone, not of its
 * alignment, of the other blocks of the call or of scheduling.  Two launches (tiles, then one workgroup a block), enqueues only,
 * no workgroup waits for another.  d_n[b] > h_cap[b] is the block's SHAFA_OUTSIDE_MODULE through shafa_hipd_finish: no byte of
 * the block is read and its record is twelve zeros.
 * Argument errors return with nothing enqueued (checked before HIP is touched).  _quant_dev and _round_dev: the corresponding
 * hist entry's checks in its order for the arguments they share (NULL b, d_in or d_n; elem; nblocks <= 0: SHAFA_SUCCESS; nblocks
 * past the batch's; NULL h_cap; capacities past 2^64 bytes or 2^31 tiles: SHAFA_LACK_OF_MEMORY; NULL h_in_off, d_in or an offset
 * that is no multiple of elem; the steps and bounds, or the widths and kept bits), then NULL d_stat.  shafa_hipd_error_dev: NULL
 * d_a or d_ref or a d_a that is no multiple of 16, and elem; then shafa_hipd_compare_dev's checks of side a in its order (NULL b
 * or d_n; nblocks; NULL h_a_off or h_cap; an h_a_off[b] that is no multiple of 16); the capacities as above; NULL h_ref_off, d_ref
 * or an h_ref_off[b] that is no multiple of elem; then, each SHAFA_OUTSIDE_MODULE: NULL h_mant or a width that is not the
 * format's, NULL d_stat, NULL h_abs or h_rel, an h_abs[b] that is NaN or < 0, an h_rel[b] that is NaN, < 0 or Inf. */
#define SHAFA_ERR_WORDS 12
int shafa_hipd_error_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint32_t *h_mant, const double *h_abs,
                         const double *h_rel, const uint8_t *d_a, const uint64_t *h_a_off, const uint64_t *h_cap,
                         const uint64_t *d_n, const uint8_t *d_ref, const uint64_t *h_ref_off, uint64_t *d_stat);
int shafa_hipd_error_quant_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const double *h_step,
                               const double *h_bound, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                               const uint64_t *d_n, uint64_t *d_stat);
int shafa_hipd_error_round_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t elem, const uint32_t *h_mant,
                               const uint32_t *h_keep, const uint8_t *d_in, const uint64_t *h_in_off, const uint64_t *h_cap,
                               const uint64_t *d_n, uint64_t *d_stat);

/* ---- Byte columns of fixed-width records: the plain transposes for any width 1 .. 64 ------------------------------------
 * An RGB image is 3-byte records, an xyz point cloud 12-byte records, a binary log whatever its struct is: column j of such
 * data — byte j of every record — has a histogram of its own, which the planes of a 1-, 2-, 4- or 8-byte element mix.  Block
 * b is d_n[b] (<= h_cap[b], device resident) RECORDS of `width` = 1 .. SHAFA_RECORDS_MAX_WIDTH bytes.
 *   record side    the block's width * d_n[b] bytes at d_in (d_out) + h_in_off[b] (h_out_off[b]); the offsets are 64-bit and
 *                  need NO alignment: records are transposed where they lie.
 *   column side    column j of block b = byte j of every record: d_n[b] bytes at d_planes + h_plane_off[b * width + j].
 *                  d_planes and every column offset are multiples of 16 (the caller allocates this side).
 * shafa_hipd_split_records_dev reads the record side and writes the columns; shafa_hipd_merge_records_dev is its inverse.  At
 * width 1, 2, 4, 8 the result is byte for byte the plain plane entries' with elem = width.
 * What is read.  split reads the record side in aligned 16-byte words that each hold at least one byte of the region; no other
 * byte is touched, nothing is copied, and bytes outside the region never influence the result.  merge reads a column in aligned
 * 16-byte words that each hold at least one of its d_n[b] bytes.
 * What is written.  split writes the d_n[b] bytes of each column and nothing behind them (whole 16-byte words, single bytes
 * in the last one).  merge writes the width * d_n[b] bytes of the region and nothing else: aligned 16-byte words that lie
 * wholly inside the bytes of one pass (below), single bytes where an unaligned region puts a word across the border of two
 * passes or across an end of the region; the up to 15 bytes on either side of an unaligned region are untouched.
 * Per-block codes through shafa_hipd_finish:
 *   d_n[b] > h_cap[b]                      SHAFA_OUTSIDE_MODULE; no byte of the block is read or written, other blocks are
 *                                          unaffected.
 * One launch for all blocks, in which no workgroup waits for another: tiles of SHAFA_RECORDS_TILE records, numbered from the
 * capacities; a workgroup takes its tile through LDS in passes of SHAFA_RECORDS_PASS(width) records (at most 32 KiB), both
 * directions moving the record side in coalesced aligned words and a column in words of 16 records; a tile at or behind d_n[b]
 * exits.  The only atomic is the error word above.  The device workspace is (20 + 8 width) bytes per block plus 20.  Enqueues
 * only: d_n is never read on the host, no device-to-host copy is issued and nothing is synchronised; the one exception is the
 * batch's growth, from nblocks.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched), in the plain entries' order:
 * NULL b (first), d_in / d_out, d_planes or d_n, a width outside 1 .. SHAFA_RECORDS_MAX_WIDTH: SHAFA_OUTSIDE_MODULE; then
 * nblocks <= 0: success (the host arrays may be NULL); nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY; NULL h_cap:
 * SHAFA_OUTSIDE_MODULE; a width * h_cap[b] or their sum past 64 bits, or 2^31 tiles of SHAFA_RECORDS_TILE records or more in
 * the capacities: SHAFA_LACK_OF_MEMORY; NULL h_in_off / h_out_off or h_plane_off, a d_planes or an h_plane_off[b * width + j]
 * that is no multiple of 16: SHAFA_OUTSIDE_MODULE. */
#define SHAFA_RECORDS_MAX_WIDTH 64
#define SHAFA_RECORDS_TILE 8192 /* records; = SHAFA_PLANES_TILE */
/* the records a workgroup takes through LDS at a time: the largest power of two with PASS * width <= 32768, 8192 at the most;
 * a multiple of 16 that divides the tile */
#define SHAFA_RECORDS_PASS(width) ((width) <= 4 ? 8192 : (width) <= 8 ? 4096 : (width) <= 16 ? 2048 : (width) <= 32 ? 1024 : 512)
int shafa_hipd_split_records_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t width, const uint8_t *d_in,
                                 const uint64_t *h_in_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_planes,
                                 const uint64_t *h_plane_off);
int shafa_hipd_merge_records_dev(shafa_hipd_batch *b, void *stream, int nblocks, uint32_t width, const uint8_t *d_planes,
                                 const uint64_t *h_plane_off, const uint64_t *h_cap, const uint64_t *d_n, uint8_t *d_out,
                                 const uint64_t *h_out_off);

/* ---- Seek index: byte ranges of a file set without decoding whole blocks -------------------------------------------------
 * A .shaf has no sync markers and an RLE triple may straddle any boundary, so a decoder can only start where it is told the
 * bit offset, the RLE state and the decoded offset.  A seek index tells it: one CHECKPOINT every `span` symbols of every
 * block's SF-decoded bytes (the original for a mode-N .shaf, the .rle bytes for a mode-R one; for a .rle + .freq set the grid
 * runs over the .rle bytes themselves).  `span` is a power of two, 256 .. 8192.  A block of n symbols has
 * max(1, ceil(n / span)) checkpoints; checkpoint k describes the position just in front of symbol k * span of the block.
 * A checkpoint is 16 bytes, two little-endian 64-bit words:
 *   w0 bits  0..47   bit offset, within the block's .shaf payload, of the code of symbol k * span (the encoder's bit order:
 *                    MSB first); 8 * k * span for a .rle + .freq set
 *      bits 48..55   pending symbol: the RLE byte at k * span - 1; meaningful only when the state is 2 (0 otherwise)
 *      bits 56..57   RLE state in front of the symbol: 0 = outside a triple, 1 = the byte before was the escape 0, 2 = the next
 *                    byte is a count.  Always 0 without SHAFA_SEEK_RLE
 *      bits 58..63   0
 *   w1               decoded offset, within the block, of the first output byte produced by bytes at or behind the checkpoint
 *                    (a run is charged to its COUNT byte; a count of 0 acts as 1); k * span without SHAFA_SEEK_RLE
 * Checkpoint 0 is {0, 0}.  The blocks' checkpoints lie one after the other in one device array (block b's first one at index
 * h_ckpt_first[b], in checkpoints); the array is plain data that a caller may keep, copy and hand back later.
 *
 * shafa_hipd_seek_index_dev builds the checkpoints of nblocks blocks from their SF-decoded bytes: block b's are the d_in_n[b]
 * (<= h_in_cap[b], device resident) bytes at d_in + h_in_off[b] — a region of shafa_hipd_sf_decode_dev, or a .rle payload
 * gathered by shafa_hipd_unpack_payloads; d_in and every offset are multiples of 16.  flags: SHAFA_SEEK_SF = the bit
 * offsets are sums of d_tables[b].len[] over the bytes (else 8 a byte, d_tables is not looked at); SHAFA_SEEK_RLE = the bytes
 * are RLE bytes.  Block b's region of d_ckpt, from checkpoint h_ckpt_first[b], holds max(1, ceil(h_in_cap[b] / span))
 * checkpoints; max(1, ceil(d_in_n[b] / span)) are written.  d_out_n[b] = the block's decoded size (what
 * shafa_hipd_rle_decoded_size_dev leaves with SHAFA_SEEK_RLE, d_in_n[b] without).  d_status[b] = SHAFA_SEEK_UNINDEXED when
 * SHAFA_SEEK_SF is set and the block's table holds a code of more than 32 bits or one of its bytes has no code: such a block
 * gets checkpoint 0 only and is read by the block decoders; else 0.  Per-block codes through shafa_hipd_finish:
 *   d_in_n[b] > h_in_cap[b]                SHAFA_OUTSIDE_MODULE, d_out_n[b] = 0, checkpoint 0 only (no byte of the block is read);
 *   with SHAFA_SEEK_RLE, the bytes end inside a {0, symbol, count} triple or decode to more than SHAFA_RLE_DECODE_MAX
 *                                          SHAFA_FILE_UNRECOGNIZABLE, d_out_n[b] = 0 (as shafa_hipd_rle_decoded_size_dev).
 * Two launches — one wave per span, then one workgroup per block — in which no workgroup waits for another and no atomic is
 * used: the result does not depend on scheduling.  The device workspace is 16 bytes per span of the capacities plus 28 bytes
 * per block.  Enqueues only: nothing is read on the host or synchronised; the one exception is the batch's growth.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_in, d_in_n, d_ckpt,
 * d_status or d_out_n, a span that is no power of two in 256 .. 8192, unknown flags, SHAFA_SEEK_SF without d_tables:
 * SHAFA_OUTSIDE_MODULE; then nblocks <= 0: success; nblocks > the batch's max_blocks, or 2^31 spans or more in the capacities:
 * SHAFA_LACK_OF_MEMORY; NULL h_in_off, h_in_cap or h_ckpt_first, a d_in or h_in_off[b] that is no multiple of 16:
 * SHAFA_OUTSIDE_MODULE. */
#define SHAFA_SEEK_SF 1
#define SHAFA_SEEK_RLE 2
#define SHAFA_SEEK_UNINDEXED 1u
int shafa_hipd_seek_index_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_in, const uint64_t *h_in_off,
                              const uint64_t *h_in_cap, const uint64_t *d_in_n, const shafa_code_table *d_tables, uint32_t span,
                              int flags, const uint64_t *h_ckpt_first, uint64_t *d_ckpt, uint32_t *d_status, uint64_t *d_out_n);

/* The ranged decoder.  The file set is described by host arrays of nblocks entries — block b's payload is the h_pay_n[b]
 * bytes at d_file + h_pay_off[b] (the .shaf or the .rle file where it lies, any alignment, file_n bytes in all), it has
 * h_n_symbols[b] symbols and its checkpoints start at h_ckpt_first[b] of d_ckpt — and by d_tables (SHAFA_SEEK_SF: what
 * shafa_hipd_unpack_cod leaves), span and flags as the index was built with.  Item i reads the bytes whose decoded offset
 * within block h_item_block[i] lies in [h_item_lo[i], h_item_hi[i]) and writes them to d_out + h_item_dst[i] + (offset - lo);
 * h_item_first[i] .. h_item_last[i] are the checkpoints of that block whose spans produce them (first: the last checkpoint
 * whose decoded offset is <= lo; last: the last one whose decoded offset is < hi).  Every span of every item is decoded on
 * its own, 64 spans of one block to a workgroup: its symbols from the checkpoint's bit offset, through the RLE machine from
 * the checkpoint's state and pending symbol with SHAFA_SEEK_RLE, until the span or the range ends.  No payload byte outside
 * [h_pay_off[b], + h_pay_n[b]) is read and no byte outside [dst, dst + hi - lo) is written, whatever the files and the index
 * hold.  Conditions that files other than the indexed ones can cause set SHAFA_FILE_UNRECOGNIZABLE for the ITEM (item i's
 * code is word i of shafa_hipd_finish) and end that span's writing: a window that matches no code, a walk past the payload's
 * end, a span whose end (bit offset, decoded offset, RLE state) disagrees with the next checkpoint, a block that ends inside
 * a triple.  A block whose table holds a code of more than 32 bits: SHAFA_OUTSIDE_MODULE for its items, nothing written.
 * One launch, no workgroup waits for another, no atomics; the device workspace is 32 bytes per block and per item plus 8
 * bytes per span read.  Enqueues only, as shafa_hipd_seek_index_dev.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_ckpt or d_out, a NULL
 * d_file with file_n > 0, a bad span or flags, SHAFA_SEEK_SF without d_tables: SHAFA_OUTSIDE_MODULE; then nitems <= 0:
 * success; nitems or nblocks > the batch's max_blocks, or 2^31 spans or more: SHAFA_LACK_OF_MEMORY; a NULL host array,
 * nblocks <= 0, a payload outside [0, file_n), an item whose block, checkpoints (first <= last < the block's count) or range
 * (lo <= hi, dst + hi - lo <= out_n) is out of bounds: SHAFA_OUTSIDE_MODULE. */
int shafa_hipd_read_spans_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_file, uint64_t file_n,
                              const uint64_t *h_pay_off, const uint64_t *h_pay_n, const uint64_t *h_n_symbols,
                              const uint64_t *h_ckpt_first, const shafa_code_table *d_tables, uint32_t span, int flags,
                              const uint64_t *d_ckpt, int nitems, const int *h_item_block, const uint64_t *h_item_first,
                              const uint64_t *h_item_last, const uint64_t *h_item_lo, const uint64_t *h_item_hi,
                              const uint64_t *h_item_dst, uint8_t *d_out, uint64_t out_n);

/* The Shannon-Fano sizes of blocks without encoding them: d_out_n[b] = the d_out_n[b] shafa_hipd_sf_encode_dev leaves for a
 * block whose histogram is d_freq[b * 256 ..] (what shafa_hipd_hist256 or shafa_hipd_rle_encoded_hist_dev leaves), encoded
 * with d_tables[b] into room enough: ceil(sum over s of d_freq[b * 256 + s] * len[s] / 8), the bits summed in 64 bits.
 * Per-block codes through shafa_hipd_finish, by binary_coding's rules:
 *   every code of the table is empty       size 0 and success (a block of one symbol);
 *   a symbol with a count and no code, in a table that holds a code
 *                                          SHAFA_FILE_UNRECOGNIZABLE, d_out_n[b] = 0;
 *   the bits do not fit 64 bits            SHAFA_OUTSIDE_MODULE, d_out_n[b] = 0 (never for a block's own histogram).
 * One workgroup per block.  Enqueues only, as shafa_hipd_sf_build_codes: nothing is read on the host or synchronised.
 * Argument errors return from the call with nothing enqueued (checked before HIP is touched): NULL b, d_freq, d_tables or
 * d_out_n: SHAFA_OUTSIDE_MODULE; nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY; nblocks <= 0: success. */
int shafa_hipd_sf_encoded_size_dev(shafa_hipd_batch *b, void *stream, int nblocks, const uint64_t *d_freq,
                                   const shafa_code_table *d_tables, uint64_t *d_out_n);

/* ---- Files in device memory: .rle, .shaf, .cod and .freq assembled from what the entries above leave -------------------
 * Each call writes ONE contiguous file at d_dst: every byte equals what the C host writes for the same sizes, tables and
 * counts (host/modules.c's framing around host/formats.c's shafa_cod_format / shafa_freq_format) — empty codes, 255-bit
 * codes, all-empty tables, counts of 0 and of 2^64 - 1, runs of equal counts (repeat = empty field), payloads of 0 bytes
 * ("@0@") and a single block included.  *d_dst_n (device) = the file's length.
 * Enqueues only, as shafa_hipd_sf_encode_dev: device sizes, tables and counts are never read on the host, no device-to-host
 * copy is issued and nothing is synchronised; the one exception is the batch's growth, from nblocks and the host capacities.
 * Errors, reported by shafa_hipd_finish (the first error per block is kept, as for every entry):
 *   d_src_n[b] > h_src_cap[b]              SHAFA_OUTSIDE_MODULE on block b, *d_dst_n = 0;
 *   a file longer than dst_cap             SHAFA_LACK_OF_MEMORY on block 0, *d_dst_n = the length the file needs.
 * In both cases nothing at all is written to d_dst: the sizes are checked before any byte moves.  Nothing is ever written
 * outside [d_dst, d_dst + min(dst_cap, *d_dst_n)).
 * Argument errors return SHAFA_OUTSIDE_MODULE from the call with nothing enqueued (checked before HIP is touched): a NULL
 * batch or device array, nblocks < 1, a mode other than 'R' / 'N', an unknown framing, d_src + h_src_off[b] not a multiple
 * of 16.  nblocks > the batch's max_blocks: SHAFA_LACK_OF_MEMORY.
 * The packs look at sizes only, not at the error words of earlier calls: a file is meaningful when shafa_hipd_finish reports
 * success for the whole chain (F -> T -> C -> packs).  d_dst needs no alignment. */
#define SHAFA_FRAME_RAW 0     /* .rle: payloads back to back (f.c:307)                                   */
#define SHAFA_FRAME_SHAF 1    /* .shaf: "@<n>", then "@<size>@" + payload per block (c.c:351,256-258)   */

/* Host-only upper bounds of a file, for sizing d_dst (no GPU needed; 0 for nblocks < 1 or an unknown framing).
 *   payloads: RAW sum(cap_b); SHAF 1 + digits(nblocks) + sum(2 + digits(cap_b) + cap_b)
 *   .cod:     3 + digits(nblocks) + nblocks * (22 + 256 * 255 + 255) + 2    (any table: <= 65 535 code characters)
 *   .freq:    3 + digits(nblocks) + nblocks * (22 + 256 * 20 + 255) + 2     (256 fields of <= 20 digits)        */
size_t shafa_hip_pack_payloads_max(int nblocks, const uint64_t *h_src_cap, int framing);
size_t shafa_hip_pack_cod_max(int nblocks);
size_t shafa_hip_pack_freq_max(int nblocks);

/* Block b's d_src_n[b] (<= h_src_cap[b]) bytes at d_src + h_src_off[b] -> one file at d_dst, framed by `framing`. */
int shafa_hipd_pack_payloads(shafa_hipd_batch *b, void *stream, int nblocks, int framing, const uint8_t *d_src,
                             const uint64_t *h_src_off, const uint64_t *h_src_cap, const uint64_t *d_src_n, uint8_t *d_dst,
                             uint64_t dst_cap, uint64_t *d_dst_n);
/* "@<mode>@<n>", then "@<d_sizes[b]>@" + the table's "c0;c1;...;c255" per block, then "@0" (t.c:302,353-361,395-396).
 * d_tables: nblocks tables in device memory (what shafa_hipd_sf_build_codes leaves). */
int shafa_hipd_pack_cod(shafa_hipd_batch *b, void *stream, int nblocks, char mode, const uint64_t *d_sizes,
                        const shafa_code_table *d_tables, uint8_t *d_dst, uint64_t dst_cap, uint64_t *d_dst_n);
/* "@<mode>@<n>", then "@<d_sizes[b]>@" + make_freq's text of d_freq[b*256 ..] per block, then "@0" (f.c:89-119). */
int shafa_hipd_pack_freq(shafa_hipd_batch *b, void *stream, int nblocks, char mode, const uint64_t *d_sizes,
                         const uint64_t *d_freq, uint8_t *d_dst, uint64_t dst_cap, uint64_t *d_dst_n);

/* ---- Many files per call: the packs above, segmented ------------------------------------------------------------------
 * File f is blocks h_first[f] .. h_first[f] + h_count[f] - 1 of the call's block arrays (files may list any blocks, the
 * same block in several files included); it is written at d_dst + h_dst_off[f] with room for h_dst_cap[f] bytes, its length
 * goes to d_dst_n[f] (device).  Each file's bytes equal what the single-file pack writes for that file's blocks alone, its
 * head carrying the file's block count (and for .cod / .freq its own mode h_modes[f]).  Enqueue only, as the packs.
 * Errors, per file (reported by shafa_hipd_finish):
 *   d_src_n[b] > h_src_cap[b]              SHAFA_OUTSIDE_MODULE on block b, d_dst_n[f] = 0 for every file that lists b;
 *   file f longer than h_dst_cap[f]        SHAFA_LACK_OF_MEMORY on block h_first[f], d_dst_n[f] = the length it needs.
 * A refused file has no byte of its region written; every other file of the call is written normally.  Overlapping
 * destination regions are the caller's error; destinations need no alignment.
 * Argument errors return SHAFA_OUTSIDE_MODULE with nothing enqueued (checked before HIP is touched): a NULL batch or array,
 * nfiles < 1, h_count[f] < 1, a block range outside [0, the batch's max_blocks), a mode other than 'R' / 'N', an unknown
 * framing, d_src + h_src_off[b] not a multiple of 16 for a listed block.  More than 2^31 - 1 blocks over all files:
 * SHAFA_LACK_OF_MEMORY.  The host arrays indexed by block hold max(h_first[f] + h_count[f]) entries. */
int shafa_hipd_pack_payloads_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                                   int framing, const uint8_t *d_src, const uint64_t *h_src_off, const uint64_t *h_src_cap,
                                   const uint64_t *d_src_n, uint8_t *d_dst, const uint64_t *h_dst_off,
                                   const uint64_t *h_dst_cap, uint64_t *d_dst_n);
int shafa_hipd_pack_cod_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                              const char *h_modes, const uint64_t *d_sizes, const shafa_code_table *d_tables,
                              uint8_t *d_dst, const uint64_t *h_dst_off, const uint64_t *h_dst_cap, uint64_t *d_dst_n);
int shafa_hipd_pack_freq_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_count,
                               const char *h_modes, const uint64_t *d_sizes, const uint64_t *d_freq,
                               uint8_t *d_dst, const uint64_t *h_dst_off, const uint64_t *h_dst_cap, uint64_t *d_dst_n);

/* ---- Files in device memory, parsed: the inverse of the packs -----------------------------------------------------------
 * .cod / .rle.freq / .shaf files at d_* (any alignment, lengths known on the host) -> the sizes, tables and payload
 * positions that shafa_hipd_sf_decode_dev / _rle_decode_dev take, by the C host's rules (host/modules.c read_header,
 * read_block, shaf_read_u64; host/formats.c shafa_cod_parse).  Enqueue only, as the packs: device sizes are never read on
 * the host, no device-to-host copy is issued and nothing is synchronised (the one exception: the batch's growth, from
 * max_blocks / nblocks, the file lengths and the host capacities).  Nothing is ever written outside the caller's arrays of
 * max_blocks (nblocks) entries, d_info's SHAFA_UNPACK_INFO_WORDS words and the destination regions.
 * Errors, reported by shafa_hipd_finish (first error per block kept):
 *   a bad header ("@<mode>@<digits>" with a count <= remaining bytes / 3; "@" + digits for .shaf)   SHAFA_FILE_STREAM_FAILED
 *                                                                                                  on block 0;
 *   block b's frame fails read_block (a size of >= 1 digit between two '@', then 1 .. max field bytes and a following '@';
 *   max field = 33 151 for .cod, 5 375 for .freq), its .shaf header fails shaf_read_u64 ('@', 1 .. 20 digits, '@'), or its
 *   payload runs past the end of its file (.shaf; .rle of rle_n bytes)                              SHAFA_FILE_STREAM_FAILED
 *                                                                                                  on block b;
 *   block b's .cod text fails shafa_cod_parse (only '0', '1', ';' up to a NUL byte; exactly 256 fields of <= 255 bits)
 *                                                                 SHAFA_FILE_UNRECOGNIZABLE on block b, all-empty table.
 * A .shaf failure on block b replaces a table error on the same block, whichever call was enqueued first (the host reads
 * the .shaf header and payload before the .cod text).  Blocks after the first framing failure get size 0, offset 0 and an
 * all-empty table, and report nothing.  The mode character
 * is recorded, not judged: the caller applies d.c:678 (R, or N without RLE decoding) or 'R' for .freq.  The .shaf count is
 * read but the .cod's count wins (d.c:676); bytes after the last payload and the .cod's "@0" tail are not looked at.
 * Several faults: the C host's answer depends on how far its pipeline reads ahead (a framing error up to `depth` blocks on
 * pre-empts an earlier block's table or decode error); these calls report every block's own first fault, so a caller that
 * takes the first error in block order (shafa.decompress_files) matches the host on files with a single fault.
 * Argument errors return SHAFA_OUTSIDE_MODULE with nothing enqueued (checked before HIP is touched): a NULL batch or array,
 * max_blocks / nblocks < 1, a NULL file with a length > 0, d_dst + h_dst_off[b] not a multiple of 16.  max_blocks / nblocks
 * > the batch's max_blocks: SHAFA_LACK_OF_MEMORY. */
#define SHAFA_UNPACK_INFO_WORDS 8
#define SHAFA_UNPACK_INFO_STATUS 0     /* SHAFA_SUCCESS, or SHAFA_FILE_STREAM_FAILED for a bad header            */
#define SHAFA_UNPACK_INFO_MODE 1       /* the header's mode character (0 when the file has none)                 */
#define SHAFA_UNPACK_INFO_COUNT 2      /* the header's block count (read_u64: unbounded digits, wrapping)         */
#define SHAFA_UNPACK_INFO_INDEXED 3    /* min(count, max_blocks): the blocks looked at                            */
#define SHAFA_UNPACK_INFO_FRAMED 4     /* the blocks before the first framing failure                             */
#define SHAFA_UNPACK_INFO_MAX_SIZE 5   /* the largest size among them                                             */

/* .cod of cod_n bytes -> d_info, d_sizes[b] (the "@<size>@" number: the block's symbol count) and d_tables[b] (the layout of
 * shafa_hipd_sf_build_codes, which shafa_hipd_sf_decode_dev takes as it lies), for b < max_blocks.  A text with more blocks
 * than max_blocks is indexed up to max_blocks: with max_blocks = cod_n / 258 + 1 (a parsable block takes >= 258 bytes) a
 * longer count always leaves a failing block among those indexed. */
int shafa_hipd_unpack_cod(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_cod, uint64_t cod_n,
                          uint64_t *d_info, uint64_t *d_sizes, shafa_code_table *d_tables);
/* .rle.freq of freq_n bytes (framing only, as rle_decompress reads it) -> d_info, and block b's .rle payload
 * [d_off[b], d_off[b] + d_n[b]) in a .rle file of rle_n bytes.  max_blocks = freq_n / 4 + 1 covers any count likewise. */
int shafa_hipd_unpack_rle_freq(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_freq, uint64_t freq_n,
                               uint64_t rle_n, uint64_t *d_info, uint64_t *d_off, uint64_t *d_n);
/* .freq or .rle.freq of freq_n bytes, its counts parsed (Module T's input, as get_shafa_codes reads it) -> d_info, d_sizes[b]
 * (the "@<size>@" number) and d_counts[b * 256 + s] (the layout shafa_hipd_hist256 leaves, which shafa_hipd_sf_build_codes and
 * shafa_hipd_pack_freq take as it lies), for b < max_blocks.  Header and frames as unpack_rle_freq (max field 5 375), without
 * a .rle to measure against.  Block b's text follows shafa_freq_parse (host/formats.c): cut at its first NUL byte, it holds
 * 256 fields of digits separated by exactly 255 ';'; field 0 is not empty, an empty field repeats the nearest non-empty one
 * before it, a field has any number of digits and its value wraps modulo 2^64.  A text that fails this:
 * SHAFA_FILE_UNRECOGNIZABLE on block b and 256 zero counts; the blocks after it are parsed all the same (a block's own fault,
 * not a framing failure).  Blocks after the first framing failure get size 0 and 256 zero counts, and report nothing. */
int shafa_hipd_unpack_freq(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_freq_text, uint64_t freq_n,
                           uint64_t *d_info, uint64_t *d_sizes, uint64_t *d_counts /* max_blocks x 256 */);
/* .shaf of shaf_n bytes -> block b's payload [d_off[b], d_off[b] + d_n[b]) for the first min(*d_count, max_blocks) blocks
 * (d_count: the .cod's count, e.g. d_info + SHAFA_UNPACK_INFO_INDEXED of shafa_hipd_unpack_cod).  The headers form a
 * dependent chain: one wave walks them, about one memory latency per block. */
int shafa_hipd_unpack_shaf(shafa_hipd_batch *b, void *stream, int max_blocks, const uint8_t *d_shaf, uint64_t shaf_n,
                           const uint64_t *d_count, uint64_t *d_off, uint64_t *d_n);
/* Block b's payload [d_file + d_off[b], + d_n[b]) -> d_dst + h_dst_off[b] (16-aligned regions of h_dst_cap[b] bytes, what the
 * decoders take).  d_n[b] > h_dst_cap[b], or a payload outside [0, file_n): SHAFA_OUTSIDE_MODULE on block b, nothing written
 * for it.  Moved by the packs' kernels (whole aligned 16-byte destination words, bytes at the ends). */
int shafa_hipd_unpack_payloads(shafa_hipd_batch *b, void *stream, int nblocks, const uint8_t *d_file, uint64_t file_n,
                               const uint64_t *d_off, const uint64_t *d_n, uint8_t *d_dst, const uint64_t *h_dst_off,
                               const uint64_t *h_dst_cap);

/* ---- Many files per call, parsed: the parses above, segmented -----------------------------------------------------------
 * File f's bytes are at base + h_*_off[f], h_*_n[f] of them (any alignment); its blocks take slots h_first[f] ..
 * h_first[f] + h_max_blocks[f] - 1 of the call's per-slot arrays and of the batch's error words, and its record goes to
 * d_info + f * SHAFA_UNPACK_INFO_WORDS.  Every slot's outputs and error word, and every file's record, equal what the
 * single-file entry writes for that file alone with max_blocks = h_max_blocks[f] (header rules, first framing failure, the
 * .shaf failure over a table error, zeroed slots after it), except that payload offsets are relative to the call's base:
 * d_shaf, or the .rle base that h_rle_off[f] is measured from.  So shafa_hipd_unpack_payloads gathers every file's payloads
 * in one call (d_file = that base, file_n = the end of the last file).  A fault in one file changes nothing in another's
 * slots or record.  unpack_shaf_files reads file f's block count at d_count[f * SHAFA_UNPACK_INFO_WORDS]: pass
 * d_info + SHAFA_UNPACK_INFO_INDEXED of unpack_cod_files.  Enqueue only, with the same exception as the entries above.
 * Argument errors return SHAFA_OUTSIDE_MODULE with nothing enqueued (checked before HIP is touched): a NULL batch or array,
 * nfiles < 1, h_max_blocks[f] < 1, a slot range outside [0, the batch's max_blocks), two files' slot ranges that overlap,
 * a NULL base with a length > 0.  More than 2^31 - 1 slots or 4 KiB text chunks: SHAFA_LACK_OF_MEMORY. */
int shafa_hipd_unpack_cod_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_max_blocks,
                                const uint8_t *d_text, const uint64_t *h_text_off, const uint64_t *h_text_n,
                                uint64_t *d_info, uint64_t *d_sizes, shafa_code_table *d_tables);
int shafa_hipd_unpack_rle_freq_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first,
                                     const int *h_max_blocks, const uint8_t *d_text, const uint64_t *h_text_off,
                                     const uint64_t *h_text_n, const uint64_t *h_rle_off, const uint64_t *h_rle_n,
                                     uint64_t *d_info, uint64_t *d_off, uint64_t *d_n);
int shafa_hipd_unpack_shaf_files(shafa_hipd_batch *b, void *stream, int nfiles, const int *h_first, const int *h_max_blocks,
                                 const uint8_t *d_shaf, const uint64_t *h_shaf_off, const uint64_t *h_shaf_n,
                                 const uint64_t *d_count, uint64_t *d_off, uint64_t *d_n);

/* Synchronise `stream`, return the first per-block error of the calls enqueued since the last
 * finish (SHAFA_SUCCESS if none).  h_block_err (nblocks ints, may be NULL) receives every block's code. */
int shafa_hipd_finish(shafa_hipd_batch *b, void *stream, int nblocks, int *h_block_err);

/* Synthetic byte streams for bench/tests (no reference counterpart; same stream as the oracle's
 * orc_gen_bytes): byte i = map[r16(seed, first_index + i)] or r16 >> 8 when d_map65536 == NULL. */
int shafa_hipd_gen_bytes(void *stream, uint64_t seed, uint64_t first_index,
                         const uint8_t *d_map65536, uint8_t *d_out, size_t n);

/* =================================================================================================
 * Layer 3 — bounded in-order block pipeline (host buffers, asynchronous).
 *
 * Stands where the reference's drivers start one thread per block and join them in order
 * (multithread.c:126-194 create, :70-87 ordered write chain; callers f.c:231-356, c.c:383-411,
 * d.c:330-345, d.c:690-740).  A pipe owns n_slots slots; each slot has a HIP stream, pinned host
 * input/output buffers and device buffers.  Usage per block: fill shafa_pipe_in(slot), submit, and
 * later wait on the slots in submission order.  Blocks in different slots overlap: host read,
 * H2D copy, kernels, D2H copy and host write of neighbouring blocks run concurrently, with at
 * most n_slots blocks in flight (the reference's read-ahead is unbounded, c.c:383).
 * ================================================================================================= */
typedef struct shafa_pipe shafa_pipe;

enum shafa_pipe_op {
    SHAFA_OP_HIST = 1,           /* make_freq of the input (f.c:325)                                  */
    SHAFA_OP_RLE_ENCODE = 2,     /* block_compression + make_freq of the RLE bytes (f.c:248,310)      */
    SHAFA_OP_SF_ENCODE = 3,      /* compress_to_buffer (c.c:91-237)                                   */
    SHAFA_OP_SF_DECODE = 4,      /* create_tree + shafa_block_decompressor (d.c:565-569)              */
    SHAFA_OP_RLE_DECODE = 5,     /* rle_block_decompressor (d.c:116-197)                              */
    SHAFA_OP_SF_RLE_DECODE = 6,  /* process_shafa_decomp with RLE (d.c:558-590), fused on the device  */
    SHAFA_OP_FTC = 7             /* Modules F and C on ONE residency of the block, Module T on the host in between:
                                    see "F -> T -> C" below                                                            */
};
#define SHAFA_PIPE_INPUT_HIST 1  /* with SHAFA_OP_RLE_ENCODE / SHAFA_OP_FTC: also the histogram of the input (-c f)  */
#define SHAFA_PIPE_FTC_RLE 2     /* SHAFA_OP_FTC: run block_compression (the block may be encoded from its RLE bytes) */
#define SHAFA_PIPE_FTC_PLAIN 4   /* SHAFA_OP_FTC: the block may be encoded as it is (tile histograms of the input)    */

typedef struct shafa_pipe_result {
    const uint8_t *out;          /* the slot's pinned result buffer (valid until the slot is reused)  */
    size_t out_n;                /* result bytes                                                      */
    size_t mid_n;                /* SF_RLE_DECODE: bytes after the SF stage                           */
    uint64_t freq[256];          /* HIST: of the input; RLE_ENCODE: of the RLE bytes                  */
    uint64_t freq_in[256];       /* RLE_ENCODE with SHAFA_PIPE_INPUT_HIST: of the input               */
} shafa_pipe_result;

int shafa_pipe_create(int n_slots, shafa_pipe **out);
void shafa_pipe_destroy(shafa_pipe *p);
int shafa_pipe_slots(const shafa_pipe *p);
int shafa_pipe_slot_device(const shafa_pipe *p, int slot);      /* the device the slot's work runs on */

/* Pinned input buffer of an idle slot, grown to hold `bytes`; NULL if the slot is busy or on failure. */
uint8_t *shafa_pipe_in(shafa_pipe *p, int slot, size_t bytes);

/* Enqueue `op` on the first in_n bytes of the slot's input buffer and return without waiting.
 * table: SF ops; n_symbols: SF decodes; out_cap: SF_ENCODE result capacity (the other ops size
 * their own results: 2n+3 for RLE_ENCODE, 64 MiB + 1 KiB for RLE decodes).  Errors of the block,
 * including malformed tables, are reported by shafa_pipe_wait so that they surface in block order. */
int shafa_pipe_submit(shafa_pipe *p, int slot, int op, size_t in_n, const shafa_code_table *table,
                      size_t n_symbols, size_t out_cap, int flags);

/* Wait for the slot's block, fetch its result into the pinned output buffer, mark the slot idle.
 * Returns the block's _modules_error number. */
int shafa_pipe_wait(shafa_pipe *p, int slot, shafa_pipe_result *res);

/* ---- F -> T -> C on one residency (the default `shafa file -b m|M`, shafa.c:293-298 with 157-198) ----------------------
 * The reference's default run reads a block in Module F, writes its .rle, and reads that again in Module C.  Here the block
 * is uploaded ONCE:
 *   shafa_pipe_submit(p, slot, SHAFA_OP_FTC, in_n, NULL, 0, 0, flags)   F on the device: with SHAFA_PIPE_FTC_RLE
 *        block_compression + make_freq of the RLE bytes (shafa_hipd_rle_encode_tiles: the 32 KiB tile histograms of the RLE
 *        bytes stay on the device), with SHAFA_PIPE_FTC_PLAIN / SHAFA_PIPE_INPUT_HIST make_freq of the input and its tile
 *        histograms (block 0, whose RLE size decides for the file, f.c:250-258, asks for both)
 *   shafa_pipe_wait(p, slot, &res)          res.out / out_n = the RLE bytes (for the .rle file), res.freq / freq_in; the
 *        slot stays reserved: the caller builds the block's codes (Module T) from the histogram of what will be encoded
 *   shafa_pipe_ftc_encode(p, slot, use_rle, &table, out_cap)   Module C from the bytes already on the device
 *        (shafa_hipd_sf_encode_tiles with the tile histograms of stage one)
 *   shafa_pipe_wait(p, slot, &res)          res.out / out_n = the .shaf payload (a second pinned buffer: the RLE bytes of
 *        the first wait stay valid until the slot is reused); the slot is idle again. */
int shafa_pipe_ftc_encode(shafa_pipe *p, int slot, int use_rle, const shafa_code_table *table, size_t out_cap);

/* ---- Groups: several consecutive blocks of a file in one slot -------------------------------------------------------------
 * One launch per block costs the submitting thread ~0.1 ms whatever the block's size, which is all of a file's time at the
 * reference's default block size (64 KiB, file.h).  A group puts up to SHAFA_PIPE_GROUP_MAX blocks into one slot: the caller
 * lays their inputs out in shafa_pipe_in(slot, total) at offsets that are multiples of 16, every kernel is launched once for
 * all of them, and the results come back together.  Same ops, same per-block results and error codes as the single-block
 * calls; a slot holds either a single block or a group. */
#define SHAFA_PIPE_GROUP_MAX 256

typedef struct shafa_pipe_block {
    size_t in_off, in_n;                 /* the block inside the slot's input buffer                               */
    const shafa_code_table *table;       /* SF ops                                                                 */
    size_t n_symbols;                    /* SF decodes                                                             */
    size_t out_cap;                      /* SF_ENCODE result capacity                                              */
} shafa_pipe_block;

int shafa_pipe_submit_group(shafa_pipe *p, int slot, int op, int nblocks, const shafa_pipe_block *blocks, int flags);

/* res[i] / block_rc[i]: block i's result and its _modules_error number (results of blocks behind a failed block are still
 * valid: the caller decides where to stop, in block order).  The return value is an error of the call itself. */
int shafa_pipe_wait_group(shafa_pipe *p, int slot, int nblocks, shafa_pipe_result *res, int *block_rc);

#ifdef __cplusplus
}
#endif
#endif /* SHAFA_HIP_H */
