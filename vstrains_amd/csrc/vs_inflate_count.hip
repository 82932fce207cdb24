// Pass 1 of the member-sharded open of a BGZF pair: the members' line counts on the device, their text thrown away.  A
// translation unit of its own so that inf_member keeps ONE caller per device image: with two kernels calling it in one
// file the inliner stops inlining the decoder into either, and k_inflate of vs_inflate.hip goes from 72 VGPRs without
// scratch to 248 with (measured with -Rpass-analysis=kernel-resource-usage); apart, both compile as k_inflate always did.
#include "vs_inflate_core.h"
#include "vs_internal.h"

// k_inflate_count: every rank of a torchrun run counts the lines of its share of the members, the ranks exchange the
// counts, each then streams its own records.  The grid is sized to the device and not to the file: wavefront w takes
// members w, w + grid, w + 2 grid, ... and inflates each into ONE 64 KiB region of its own (scratch + w * 64 KiB; a
// match reads its source there, as in k_inflate), so the device memory of a pass is grid x 64 KiB whatever the file's
// size.  Decoder, range checks and CRC32 are k_inflate's; the walk over the output that makes the per-lane CRC slices
// also counts '\n' and notes '\r' and bytes >= 0x80 (inf_crc_count_part).  res[4 m ..] = status, newlines, INF_FL_*
// flags, last byte (0 for an empty member). Loops: the member loop runs ceil(n / grid) times; everything inside is
// bounded by in_len and ISIZE as in k_inflate.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 72 VGPRs, 104 SGPRs, no scratch,
// no spills, 5 312 B of LDS per workgroup of one wavefront, 7 waves per SIMD (k_inflate: 72 VGPRs, 94 SGPRs, no scratch,
// 7 waves).
__global__ void __launch_bounds__(VS_WAVE) k_inflate_count(const uint8_t *__restrict__ comp, uint64_t comp_size, uint8_t *scratch,
                                                           const vs_bgzf_member *__restrict__ dir, uint32_t n, uint32_t *__restrict__ res) {
    __shared__ InfState S;
    const uint32_t lane = threadIdx.x;
    uint8_t *o = scratch + (uint64_t)blockIdx.x * INF_MAX_ISIZE;
    inf_crc_table(&S, lane, VS_WAVE);
    for (uint32_t m = blockIdx.x; m < n; m += gridDim.x) {
        const vs_bgzf_member *e = dir + m;
        const uint32_t in_off = INF_UNI(e->in_off), in_len = INF_UNI(e->in_len);
        const uint32_t isize = INF_UNI(e->isize), crc = INF_UNI(e->crc);
        uint32_t st = INF_E_ARG, nl = 0, fl = 0, last = 0;
        if (isize <= INF_MAX_ISIZE && in_len < 65536u && (uint64_t)in_off + in_len <= comp_size) {
            st = inf_member(&S, comp + in_off, in_len, o, isize, lane, VS_WAVE);
            if (st == INF_OK) {
                INF_SYNC();
                uint32_t c = inf_crc_count_part(&S, o, isize, lane, nl, fl);
#pragma unroll
                for (uint32_t k = VS_WAVE / 2u; k; k >>= 1) {
                    c ^= __shfl_xor(c, k);
                    nl += __shfl_xor(nl, k);
                    fl |= __shfl_xor(fl, k);
                }
                if (c != crc) st = INF_E_CRC;
                if (isize) last = o[isize - 1u];
            }
        }
        if (lane == 0) {
            res[4u * m + 0u] = st;
            res[4u * m + 1u] = nl;
            res[4u * m + 2u] = fl;
            res[4u * m + 3u] = last;
        }
        INF_SYNC();  // (the next member's stores go to the region these loads read)
    }
}

void vs_launch_inflate_count(hipStream_t st, const uint8_t *comp, uint64_t comp_size, uint8_t *scratch, uint32_t grid, const vs_bgzf_member *dir,
                             uint32_t n, uint32_t *res) {
    if (n && grid) hipLaunchKernelGGL(k_inflate_count, dim3(grid < n ? grid : n), dim3(VS_WAVE), 0, st, comp, comp_size, scratch, dir, n, res);
}

