// sf_encode_dev.hip — Module C with its code tables AND its block sizes in device memory (shafa_hipd_sf_encode_dev).
//
// sfenc_launch (sf_encode.hip) reads every table on the host: to classify blocks by their longest code, to choose the
// kernel forms by the launch's longest code and to pack the look-up tables it uploads.  Here a plan kernel (one workgroup
// per block) does that on the device: it reads d_tables[b] and d_in_n[b], computes the block's longest code, writes the
// block's look-up table in the format its form reads and the block's record into a list PER FORM.  The host launches every
// form the batch could need, each over all nblocks slots of its list; a slot whose block belongs to another form holds an
// empty record (n = 0, scratch ticket, size and error word), which every encoder kernel gives up on at once (the generic
// list is compacted instead).  So a block is encoded by the kernels sfenc_launch would give it, and the bytes are the same.
//
// What the host still decides, from host arguments only: the workspace layout (descriptor bases sized for h_in_cap[b] over
// every form), grid sizes (nblocks, ceil(max h_in_cap / tile)), and the one-pass / count-scan-pack choice (sfenc_one_pass on
// nblocks instead of the per-class count: the output bytes do not depend on it).  The look-up table entries and the code
// values come from the helpers of internal.hpp that sfenc_launch uses.  Nothing is read back: no device-to-host
// copy, no synchronisation (batch_reserve and the parameter ring aside, which depend on nblocks and h_in_cap only).
#include "common.hpp"
#include "internal.hpp"

namespace {

// the forms: lists 0..3 = codes of <= 16 bits by longest code (<= 8, <= 12, 13..15, 16: the template forms of sfenc4_launch;
// count / scan / pack uses list 0 for all of them; the tile-histogram encoder two, lists 1 and 3: <= 12 bits and 13..16
// bits, see sfenc_launch_dev), 4 = 17..32 bits: one slot per block, empty records
// for the blocks of other forms.  List 5 = longer codes (the generic kernel): compacted, the blocks that have them only
// (the generic kernel loops over records x tiles, so empty records would cost it a look at every slot).
//
// Shared state the empty records rely on (a change to the encoder kernels must keep it harmless):
//   * their ticket is tickets[nblocks] / tickets2[nblocks], never zeroed: every sfe5 workgroup that meets an empty record
//     adds to it and moves on, because n = 0 leaves no tile to take;
//   * redo[b] is one flag per block for all lists: a redo-only launch of another list also visits block b's empty record
//     when b was flagged by its own list, and returns at once for the same reason (n = 0).
constexpr int NLIST = 6;
constexpr int NLIST_SLOTS = 5;                         // lists with a slot per block
constexpr int LUT_BYTES = 2048;                        // per block: the largest table a <= 32-bit form reads
constexpr u32 TILE_E3 = 8192, TILE_E6 = 32768, TILE_GEN = 1024;     // symbols per tile of sfe3 / sfe6 / sf_encode_generic
constexpr u32 GEN_GRID = 2048;                         // workgroups of the generic kernel (it loops over its tiles)

enum C1Mode { C1_SFE3 = 0, C1_ONE_PASS = 1, C1_TILES = 2 };

// host-known per block, uploaded with the launch
struct PlanBlk {
    const u8 *in;
    u8 *out;
    u64 in_cap;
    u64 out_cap;
    const u8 *thist;
    u32 desc_base;         // the block's first descriptor / tile-bits entry: ceil(in_cap / TILE_GEN) + 1 of them
    u32 pad;
};

struct PlanOut {
    EncBlk *lists;         // NLIST x nblocks records
    u8 *luts;              // LUT_BYTES per block
    u64 *desc, *desc2;     // the chains (zeroed here for the blocks that use them)
    u32 *tickets, *tickets2, *redo;   // nblocks + 1 (the last: the empty records' ticket)
    u32 *gen_plan;         // {most tiles of a generic block, generic blocks} (zeroed by the host before the plan)
    u64 *scratch_n;        // size word of the empty records
    int *scratch_err;      // error word of the empty records (never set: they have no bytes)
    u32 scratch_desc;      // descriptor index of the empty records (sfe6_scan writes one entry)
};

__global__ __launch_bounds__(256) void sfe_plan_kernel(const PlanBlk *__restrict__ pb, int nblocks, const u64 *__restrict__ d_in_n,
                                                       const shafa_code_table *__restrict__ d_tables, u64 *d_out_n, int *d_err,
                                                       PlanOut po, int c1mode, int one_pass2)
{
    __shared__ u32 lmax_sh;
    const int b = blockIdx.x, s = threadIdx.x;
    const shafa_code_table *t = d_tables + b;
    const u32 len = t->len[s];
    if (s == 0) lmax_sh = 0;
    __syncthreads();
    if (len) atomicMax(&lmax_sh, len);
    __syncthreads();
    const u32 lmax = lmax_sh;
    const PlanBlk p = pb[b];
    const u64 n = d_in_n[b];
    const bool over = n > p.in_cap;
    // 0 = nothing to encode (empty table, empty block, or a size past the block's capacity), as sfenc_launch's classes
    const int cls = (over || lmax == 0 || n == 0) ? 0 : (lmax <= 16 ? 1 : (lmax <= 32 ? 2 : 3));
    int list = -1;
    if (cls == 1 && c1mode == C1_SFE3) list = 0;
    else if (cls == 1 && c1mode == C1_TILES) list = lmax <= 12 ? 1 : 3;
    else if (cls == 1) list = lmax <= 8 ? 0 : lmax <= 12 ? 1 : lmax <= 15 ? 2 : 3;
    else if (cls == 2) list = 4;
    else if (cls == 3) list = 5;
    const bool chained = (cls == 1 && c1mode == C1_ONE_PASS) || (cls == 2 && one_pass2);

    // the look-up table, in the format sfenc_launch packs for this block's form
    u8 *lut = po.luts + (size_t)b * LUT_BYTES;
    if (cls == 1 || cls == 2) {
        const u32 cv = sfe_code_value(*t, (u32)s, len);
        if (cls == 1 && c1mode == C1_SFE3) ((u32 *)lut)[s] = sfe_entry32(cv, len);
        else if (cls == 2 && !one_pass2) ((u64 *)lut)[s] = sfe_entry64(cv, len);
        else ((u64 *)lut)[s] = sfe_entry_pair(cv, len);
    }
    const u32 tsyms = cls == 3 ? TILE_GEN : (cls == 1 && c1mode == C1_TILES ? TILE_E6 : TILE_E3);
    const u32 n_tiles = cls ? (u32)((n + tsyms - 1) / tsyms) : 0u;
    // the chains this block's kernels wait on start at zero: the one-pass forms' (32 or 8 KiB tiles, and the encode-again
    // pass's), the generic kernel's (1 KiB tiles); the region holds ceil(in_cap / 1 KiB) + 1 entries
    if (chained) {
        const u32 nd = (u32)((n + TILE_E3 - 1) / TILE_E3) + 1;
        for (u32 i = (u32)s; i < nd; i += 256) { po.desc[p.desc_base + i] = 0; po.desc2[p.desc_base + i] = 0; }
    } else if (cls == 3) {
        for (u32 i = (u32)s; i < n_tiles; i += 256) po.desc[p.desc_base + i] = 0;
    }
    if (s == 0) {
        po.tickets[b] = 0;
        po.tickets2[b] = 0;
        po.redo[b] = 0;
        if (cls == 0) d_out_n[b] = 0;
        if (over) set_error(d_err + b, SHAFA_OUTSIDE_MODULE);
    }
    if (s < NLIST_SLOTS || (s == 5 && cls == 3)) {
        EncBlk e;
        e.in = p.in;
        e.out = p.out;
        e.lut = cls == 3 ? (const void *)t : (const void *)lut;
        e.pad = 0;
        if (s == list) {
            e.n = n;
            e.out_cap = p.out_cap;
            e.out_n = d_out_n + b;
            e.err = d_err + b;
            e.desc_base = p.desc_base;
            e.n_tiles = n_tiles;
            e.ticket = (u32)b;
            e.thist = (cls == 1 && c1mode == C1_TILES) ? p.thist : nullptr;
        } else {                                       // empty record: every encoder kernel returns at once for it
            e.n = 0;
            e.out_cap = 0;
            e.out_n = po.scratch_n;
            e.err = po.scratch_err;
            e.desc_base = po.scratch_desc;
            e.n_tiles = 0;
            e.ticket = (u32)nblocks;
            e.thist = nullptr;
        }
        if (s == 5) {                                  // the generic list: the next free record
            atomicMax(po.gen_plan, n_tiles);
            po.lists[(size_t)s * nblocks + atomicAdd(po.gen_plan + 1, 1u)] = e;
        } else po.lists[(size_t)s * nblocks + b] = e;
    }
}

}  // namespace

int sfenc_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u8 *d_in, const u64 *h_in_off, const u64 *h_in_cap,
                     const u64 *d_in_n, const shafa_code_table *d_tables, u8 *d_out, const u64 *h_out_off,
                     const u64 *h_out_cap, u64 *d_out_n, const u8 *d_thist, const u64 *h_thist_off)
{
    if (nblocks <= 0) return SHAFA_SUCCESS;
    if (nblocks > bt->max_blocks) return SHAFA_LACK_OF_MEMORY;
    if ((d_thist == nullptr) != (h_thist_off == nullptr)) return SHAFA_OUTSIDE_MODULE;
    const bool tiles = d_thist != nullptr;
    u64 ndesc = 0, max_cap = 0;
    for (int b = 0; b < nblocks; ++b) {
        if ((h_in_off[b] & 15) || (h_out_off[b] & 15) || (tiles && (h_thist_off[b] & 15))) return SHAFA_OUTSIDE_MODULE;
        ndesc += ceil_div_u64(h_in_cap[b], TILE_GEN) + 1;
        if (h_in_cap[b] > max_cap) max_cap = h_in_cap[b];
    }
    const u32 scratch_desc = (u32)ndesc;
    if (++ndesc >= 0xFFFFFFFFull) return SHAFA_LACK_OF_MEMORY;

    // the forms, from host arguments only: sfenc_launch's rule on nblocks instead of its per-class counts
    const bool one_pass = sfenc_one_pass(1, nblocks), one_pass2 = sfenc_one_pass(2, nblocks);
    const int c1mode = tiles ? C1_TILES : one_pass ? C1_ONE_PASS : C1_SFE3;

    // device workspace: [header: generic plan, scratch error, scratch size][desc][desc2][tile bits][tickets][tickets2]
    // [redo][look-up tables][lists]; the parameter buffer: PlanBlk x nblocks
    const size_t nb1 = (size_t)nblocks + 1;
    size_t off = 0;
    const size_t o_hdr = off; off += 64;
    const size_t o_desc = off; off += ndesc * 8;
    const size_t o_desc2 = off; off += ndesc * 8;
    const size_t o_tbits = off; off += ndesc * 4; off = (off + 15) & ~(size_t)15;
    const size_t o_tick = off; off += nb1 * 4; off = (off + 15) & ~(size_t)15;
    const size_t o_tick2 = off; off += nb1 * 4; off = (off + 15) & ~(size_t)15;
    const size_t o_redo = off; off += nb1 * 4; off = (off + 15) & ~(size_t)15;
    const size_t o_lut = off; off += (size_t)nblocks * LUT_BYTES;
    const size_t o_list = off; off += (size_t)NLIST * nblocks * sizeof(EncBlk);
    int rc = batch_reserve(bt, st, off);
    if (rc) return rc;
    u8 *ws = (u8 *)bt->d_ws;

    const size_t stage_bytes = (size_t)nblocks * sizeof(PlanBlk);
    u8 *dpar = batch_params_begin(bt, stage_bytes);
    if (!dpar) return SHAFA_LACK_OF_MEMORY;
    ParamsScope pscope(bt, st);
    PlanBlk *hp = (PlanBlk *)batch_stage(bt, bt->par_inline ? st : bt->copy_st, stage_bytes);
    if (!hp) return SHAFA_LACK_OF_MEMORY;
    u32 dbase = 0;
    for (int b = 0; b < nblocks; ++b) {
        hp[b].in = d_in + h_in_off[b];
        hp[b].out = d_out + h_out_off[b];
        hp[b].in_cap = h_in_cap[b];
        hp[b].out_cap = h_out_cap[b];
        hp[b].thist = tiles ? d_thist + h_thist_off[b] : nullptr;
        hp[b].desc_base = dbase;
        hp[b].pad = 0;
        dbase += (u32)ceil_div_u64(h_in_cap[b], TILE_GEN) + 1;
    }
    HIP_TRY(hipMemsetAsync(ws + o_hdr, 0, 64, st));
    if ((rc = batch_params_commit(bt, st, hp, stage_bytes))) return rc;

    PlanOut po;
    po.lists = (EncBlk *)(ws + o_list);
    po.luts = ws + o_lut;
    po.desc = (u64 *)(ws + o_desc);
    po.desc2 = (u64 *)(ws + o_desc2);
    po.tickets = (u32 *)(ws + o_tick);
    po.tickets2 = (u32 *)(ws + o_tick2);
    po.redo = (u32 *)(ws + o_redo);
    po.gen_plan = (u32 *)(ws + o_hdr);
    po.scratch_err = (int *)(ws + o_hdr + 8);
    po.scratch_n = (u64 *)(ws + o_hdr + 16);
    po.scratch_desc = scratch_desc;
    hipLaunchKernelGGL(sfe_plan_kernel, dim3((u32)nblocks), dim3(256), 0, st, (const PlanBlk *)dpar, nblocks, d_in_n, d_tables,
                       d_out_n, bt->d_err, po, c1mode, (int)one_pass2);
    HIP_TRY(hipGetLastError());

    const EncBlk *lists = po.lists;
    auto list = [&](int l) { return lists + (size_t)l * nblocks; };
    const SfeRedo x = {po.desc2, po.tickets2, po.redo};
    static const u32 form_lmax[4] = {8, 12, 15, 16};   // the longest code each <= 16-bit list may hold
    const u32 tiles_e6 = (u32)ceil_div_u64(max_cap, TILE_E6), tiles_e3 = (u32)ceil_div_u64(max_cap, TILE_E3);
    // a block's size is not known here: the ragged-remainder kernels always run (one workgroup per block, gone at once
    // when the block has no remainder)
    if (c1mode == C1_TILES) {
        // Two forms, not sfenc6_launch's four: a form the batch does not use still starts its one-shot grid, ceil(max h_in_cap /
        // 32 KiB) x nblocks workgroups that return at once (~60 us at 128 x 64 MiB), and a workgroup looping over several tiles
        // makes the form in use slower by as much (measured: DESIGN 7.6).  <= 12 bits run as sfenc6_launch runs them at
        // Lmax 9..12 (<= 8 too, with windows for 12 bits), 13..16 bits as at Lmax 16 (exact for any code of <= 16 bits).
        for (int l : {1, 3})
            if (tiles_e6 && (rc = sfenc6_launch(st, list(l), nblocks, tiles_e6, form_lmax[l], true, (u32 *)(ws + o_tbits), po.desc)))
                return rc;
    } else if (c1mode == C1_ONE_PASS) {
        for (int l = 0; l < 4; ++l)
            if ((rc = sfenc4_launch(st, list(l), nblocks, po.desc, po.tickets, form_lmax[l], 7u, x))) return rc;
    } else if (tiles_e3) sfenc3_launch(st, list(0), nblocks, tiles_e3, (u32 *)(ws + o_tbits), po.desc, false);
    if (one_pass2) {
        if ((rc = sfenc4_launch_long(st, list(4), nblocks, po.desc, po.tickets, 32, 7u, x))) return rc;
    } else if (tiles_e3) sfenc3_launch(st, list(4), nblocks, tiles_e3, (u32 *)(ws + o_tbits), po.desc, true);
    const u64 gen_slots = (u64)nblocks * ceil_div_u64(max_cap, TILE_GEN);
    if (gen_slots)
        sfenc_generic_launch_dev(st, list(5), gen_slots < GEN_GRID ? (u32)gen_slots : GEN_GRID, po.desc, po.tickets,
                                 po.gen_plan);
    HIP_TRY(hipGetLastError());
    return pscope.done();
}
