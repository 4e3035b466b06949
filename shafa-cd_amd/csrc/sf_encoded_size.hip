// sf_encoded_size.hip — the Shannon-Fano size of a block from its histogram and its code table, without encoding it
// (shafa_hipd_sf_encoded_size_dev): ceil(sum_s freq[s] * len[s] / 8), with binary_coding's per-block rules as the oracle
// states them (orc_sf_encode): an all-empty table is size 0 and success; a counted symbol without a code, in a table that
// holds a code, is SHAFA_FILE_UNRECOGNIZABLE and size 0.
// One workgroup per block, a lane per symbol, a wave reduction.  Bits are summed in 128 bits (a product is at most
// 255 (2^64 - 1)), so a sum that does not fit 64 bits is seen and not wrapped: SHAFA_OUTSIDE_MODULE, size 0.  A block's own
// histogram sums to its size and cannot get there; the rule keeps the function total for hand-made counts.
#include "common.hpp"
#include "internal.hpp"

namespace {

constexpr int SFS_THREADS = 256;

__global__ __launch_bounds__(SFS_THREADS) void sf_esize_kernel(const u64 *__restrict__ freq,
                                                              const shafa_code_table *__restrict__ tables,
                                                              u64 *__restrict__ d_out_n, int *__restrict__ err)
{
    __shared__ u64 w_lo[4], w_hi[4];
    __shared__ u32 w_flag[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const u32 b = blockIdx.x;
    const u64 f = freq[(size_t)b * 256 + tid];
    const u32 len = tables[b].len[tid];
    u64 lo = f * len, hi = __umul64hi(f, (u64)len);
    // bit 0: the table holds a code; bit 1: a counted symbol has none
    const u32 flag = (__any(len != 0u) ? 1u : 0u) | (__any(f != 0 && len == 0u) ? 2u : 0u);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 ol = __shfl_xor(lo, d, 64), oh = __shfl_xor(hi, d, 64);
        lo += ol;
        hi += oh + (lo < ol ? 1u : 0u);
    }
    if (lane == 0) { w_lo[wv] = lo; w_hi[wv] = hi; w_flag[wv] = flag; }
    __syncthreads();
    if (tid == 0) {
        u64 tl = 0, th = 0;
        u32 fl = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            tl += w_lo[q];
            th += w_hi[q] + (tl < w_lo[q] ? 1u : 0u);
            fl |= w_flag[q];
        }
        u64 size = 0;
        if (fl & 1u) {
            if (fl & 2u) set_error(err + b, SHAFA_FILE_UNRECOGNIZABLE);
            else if (th) set_error(err + b, SHAFA_OUTSIDE_MODULE);
            else size = tl / 8u + ((tl & 7u) ? 1u : 0u);
        }
        d_out_n[b] = size;
    }
}

}  // namespace

int sfesize_launch_dev(Batch *bt, hipStream_t st, int nblocks, const u64 *d_freq, const shafa_code_table *d_tables, u64 *d_out_n)
{
    hipLaunchKernelGGL(sf_esize_kernel, dim3((u32)nblocks), dim3(SFS_THREADS), 0, st, d_freq, d_tables, d_out_n, bt->d_err);
    HIP_TRY(hipGetLastError());
    return SHAFA_SUCCESS;
}
