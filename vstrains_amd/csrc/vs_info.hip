// Sparse (and BGZF) pe_info / st_info: the dense text of utils/VStrains_PE_Inference.py:194-205 without the lines whose count is 0,
// written straight from the counters on the device, and the parser that reads such a file (or a dense one) back into
// (row, column, value) cells.  process_pe_info (utils/VStrains_IO.py:598-623) zeroes every key before it adds the lines,
// so the reference builds the same dict from either file.
//
// Writer, two passes over the caller's cells in the caller's order, gathered through `rank` (no permuted copy of a matrix,
// no download of one, no sort):
//   k_info_row_sizes  one workgroup per row: lines, text bytes and counter cells read of that row
//   (host)            prefix over the rows; the rows cut into blocks of whole rows of at most 256 MB of text
//   k_info_format     one workgroup per row of a block: columns in chunks of 256, the byte offset of every line from an
//                     in-order workgroup prefix sum of the line lengths (wavefront scans by DPP moves), the line stored
//                     byte by byte at its place in the block's text
// Two device / pinned buffer pairs alternate: the device formats and copies block k + 1 while the host writes block k.
// What a cell's value is and how its line reads is vs_info_core.h, shared with the host twin below.
//
// The same two passes write the files as BGZF (vs_write_info_bgzf), the sparse text or the DENSE one (VsInfoSrc::dense: the
// zero lines kept, which is the reference's own file): a block's text then stays in ONE device buffer, k_deflate
// (vs_deflate.hip, one wavefront per member of at most 0xFF00 bytes; members never span blocks) makes its members in slots,
// k_deflate_pack moves them back to back from the scan of their sizes, and only those bytes are copied to the pinned buffer
// and written -- the two buffer pairs then alternate over PACKED members.  The 28-byte EOF member ends the file.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "vs_internal.h"
#include "vs_deflate_core.h"
#include "vs_info_core.h"

namespace {

#define INFO_TPB 256u

// sizes[3 i ..] = lines, text bytes, counter cells read of the caller's row i; *flag |= 1 when a total is negative
__global__ void __launch_bounds__(INFO_TPB) k_info_row_sizes(const VsInfoSrc s, const uint64_t *__restrict__ id_off, uint64_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ flag) {
    __shared__ unsigned long long acc[3];
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    if (tid < 3u) acc[tid] = 0ull;
    __syncthreads();
    const uint32_t li = (uint32_t)(id_off[i + 1] - id_off[i]);
    uint32_t lines = 0, reads = 0;
    uint64_t bytes = 0;
    bool neg = false;
    for (uint32_t j = vs_info_first_col(s, i) + tid; j < s.n; j += INFO_TPB) {
        const int64_t v = vs_info_value(s, i, j, &reads);
        if (v < 0) neg = true;
        if (vs_info_has_line(s, v)) {
            lines++;
            bytes += vs_info_line_len(li, (uint32_t)(id_off[j + 1] - id_off[j]), (uint64_t)v);
        }
    }
    if (lines | reads) {  // (one LDS atomic per thread that saw anything; the row's totals leave through one thread)
        atomicAdd(&acc[0], (unsigned long long)lines);
        atomicAdd(&acc[1], (unsigned long long)bytes);
        atomicAdd(&acc[2], (unsigned long long)reads);
    }
    if (neg) atomicOr(flag, 1u);
    __syncthreads();
    if (tid < 3u) sizes[3ull * i + tid] = acc[tid];
}

// rows [i0, i0 + gridDim.x) of the caller's matrix into out[0, out_bytes): row i starts at row_off[i] - base.  *flag |= 2
// when a line would not fit (the counters changed between the passes): nothing is stored outside out.
__global__ void __launch_bounds__(INFO_TPB) k_info_format(const VsInfoSrc s, const uint8_t *__restrict__ ids, const uint64_t *__restrict__ id_off,
                                                          const uint64_t *__restrict__ row_off, uint32_t i0, uint64_t base, uint8_t *__restrict__ out,
                                                          uint64_t out_bytes, uint32_t *__restrict__ flag) {
    __shared__ uint32_t wave_total[INFO_TPB / VS_WAVE];
    const uint32_t i = i0 + blockIdx.x, tid = threadIdx.x, wave = tid / VS_WAVE, lane = tid % VS_WAVE;
    const uint64_t row_begin = row_off[i] - base, row_end = row_off[i + 1] - base;
    if (row_begin == row_end) return;  // (a row without a line; the same for every thread)
    const uint8_t *idi = ids + id_off[i];
    const uint32_t li = (uint32_t)(id_off[i + 1] - id_off[i]);
    uint64_t run = row_begin;
    uint32_t reads = 0;
    for (uint32_t c0 = vs_info_first_col(s, i); c0 < s.n; c0 += INFO_TPB) {
        const uint32_t j = c0 + tid;
        int64_t v = 0;
        uint32_t lj = 0, len = 0;
        if (j < s.n) {
            v = vs_info_value(s, i, j, &reads);
            if (vs_info_has_line(s, v)) {
                lj = (uint32_t)(id_off[j + 1] - id_off[j]);
                len = vs_info_line_len(li, lj, (uint64_t)v);
            }
        }
        const uint32_t incl = vs_wave_scan_add(len);
        if (lane == VS_WAVE - 1u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < INFO_TPB / VS_WAVE; w++) {
            const uint32_t t = wave_total[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        __syncthreads();
        if (len) {
            const uint64_t at = run + before + (incl - len);
            if (at + len <= row_end && row_end <= out_bytes)
                vs_info_put_line(out + at, idi, li, ids + id_off[j], lj, (uint64_t)v);
            else
                atomicOr(flag, 2u);
        }
        run += total;
    }
}

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};
struct Events {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

uint64_t text_block() {  // bytes of text per block: whole rows, one row alone may be larger (VS_TEXT_BLOCK: tests, many small blocks)
    uint64_t block = 256ull << 20;
    if (const char *ev = getenv("VS_TEXT_BLOCK")) block = std::max<uint64_t>(1u, (uint64_t)atoll(ev));
    return block;
}
// one past the last row of the block that starts at row i0
uint32_t block_end(const std::vector<uint64_t> &row_off, uint32_t n, uint32_t i0, uint64_t block) {
    uint32_t i1 = i0 + 1u;
    while (i1 < n && row_off[i1 + 1] - row_off[i0] <= block) i1++;
    return i1;
}
int pwrite_all(int fd, const uint8_t *buf, uint64_t bytes, uint64_t at) {  // 0 or errno
    while (bytes) {
        const ssize_t w = pwrite(fd, buf, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)at);
        if (w < 0 && errno == EINTR) continue;
        if (w < 0) return errno;
        buf += w, at += (uint64_t)w, bytes -= (uint64_t)w;
    }
    return 0;
}

// the checks both writers make on their host arguments
int info_check_args(vs_ctx *ctx, const char *who, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const void *counts,
                    const void *wide, const uint32_t *rank) {
    if (!path || !id_off || (n && (!ids || (!counts && !wide)))) return vs_fail(ctx, VS_E_ARG, "%s: bad argument", who);
    for (uint32_t i = 0; i < n; i++)
        if (id_off[i + 1] < id_off[i] || id_off[i + 1] - id_off[i] > 0xFFFFu) return vs_fail(ctx, VS_E_ARG, "%s: id %u: offsets must not decrease, an id has at most 65535 bytes", who, i);
    if (rank)
        for (uint32_t i = 0; i < n; i++)
            if (rank[i] >= n) return vs_fail(ctx, VS_E_RANGE, "%s: rank[%u] = %u is no node (n = %u)", who, i, rank[i], n);
    return VS_OK;
}

// rows -> prefix of the text bytes, the largest block, the totals
struct InfoPlan {
    std::vector<uint64_t> row_off;
    uint64_t block = 0, cap = 0, lines = 0, reads = 0;
    uint32_t n_blocks = 0;
    void make(const std::vector<uint64_t> &sizes, uint32_t n) {
        row_off.assign((size_t)n + 1u, 0);
        for (uint32_t i = 0; i < n; i++) {
            lines += sizes[3u * (size_t)i];
            row_off[i + 1] = row_off[i] + sizes[3u * (size_t)i + 1u];
            reads += sizes[3u * (size_t)i + 2u];
        }
        block = text_block();
        for (uint32_t i0 = 0; i0 < n;) {
            const uint32_t i1 = block_end(row_off, n, i0, block);
            if (row_off[i1] > row_off[i0]) n_blocks++;  // (a block without text is not written)
            cap = std::max(cap, row_off[i1] - row_off[i0]);
            i0 = i1;
        }
    }
};

}  // namespace

namespace {

#define INFO_MEMBER_CAP (DEF_MAX_TEXT + DEF_MEMBER_EXTRA)  // the most a member takes: its slot on the device
inline uint64_t info_members(uint64_t text_bytes) { return (text_bytes + DEF_MAX_TEXT - 1u) / DEF_MAX_TEXT; }

// The device writer.  Plain text (bgzf == false): vs_write_info_sparse.  BGZF (bgzf == true): every block's text stays on the
// device, k_deflate makes its members (members never span blocks: a block's last member is short), they are packed back to
// back from the scan of their sizes, and only those bytes are copied and written; the EOF member ends the file.
// res: [0] lines, [1] text bytes, [2] blocks, [3] cells read, [4] members, [5] file bytes.
int info_write_device(vs_ctx *ctx, const char *who, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *d_counts,
                      const int64_t *d_wide, const uint8_t *d_tile_map, const uint32_t *rank, int upper, int dense, bool bgzf, uint64_t res[6]) {
    if (!ctx) return VS_E_ARG;
    if (int rc = info_check_args(ctx, who, path, ids, id_off, n, d_counts, d_wide, rank)) return rc;
    for (int i = 0; i < 6; i++) res[i] = 0;
    Fd file;
    file.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (file.fd < 0) return vs_fail(ctx, VS_E_ARG, "cannot open %s for writing: %s", path, strerror(errno));
    const auto finish = [&](uint64_t at) -> int {  // what ends the file
        if (!bgzf) return VS_OK;
        if (const int e = pwrite_all(file.fd, vs_bgzf_eof, sizeof vs_bgzf_eof, at)) return vs_fail(ctx, VS_E_ARG, "write to %s failed: %s", path, strerror(e));
        res[5] = at + sizeof vs_bgzf_eof;
        return VS_OK;
    };
    if (!n) return finish(0);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const size_t id_bytes = (size_t)(id_off[n] - id_off[0]);
    std::vector<uint64_t> off0((size_t)n + 1u);  // (offsets from the first id's first byte)
    for (uint32_t i = 0; i <= n; i++) off0[i] = id_off[i] - id_off[0];
    VsDevBuf d_ids, d_off, d_rank, d_sizes, d_flag, d_row_off, d_text[2];
    VsDevBuf d_slots, d_msize, d_moff, d_mres, d_tmp, d_total;  // (BGZF only; d_text[1] is then not used, d_text[0] never leaves)
    VsPinnedBuf h_text[2];
    VS_HIP(ctx, d_ids.reserve(id_bytes ? id_bytes : 1u));
    VS_HIP(ctx, d_off.reserve(off0.size() * sizeof(uint64_t)));
    VS_HIP(ctx, d_sizes.reserve(3u * (size_t)n * sizeof(uint64_t)));
    VS_HIP(ctx, d_flag.reserve(sizeof(uint32_t)));
    VS_HIP(ctx, d_row_off.reserve(off0.size() * sizeof(uint64_t)));
    if (id_bytes) VS_HIP(ctx, hipMemcpyAsync(d_ids.ptr(), ids + id_off[0], id_bytes, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(d_off.ptr(), off0.data(), off0.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (rank) {
        VS_HIP(ctx, d_rank.reserve((size_t)n * sizeof(uint32_t)));
        VS_HIP(ctx, hipMemcpyAsync(d_rank.ptr(), rank, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    VS_HIP(ctx, hipMemsetAsync(d_flag.ptr(), 0, sizeof(uint32_t), st));
    VsInfoSrc src;
    src.counts = d_counts, src.wide = d_wide, src.map = d_counts ? d_tile_map : nullptr, src.rank = d_rank.as<const uint32_t>();
    src.n = n, src.T = (n + 63u) >> VS_INFO_TILE_SHIFT, src.upper = upper ? 1 : 0, src.dense = dense ? 1 : 0;
    hipLaunchKernelGGL(k_info_row_sizes, dim3(n), dim3(INFO_TPB), 0, st, src, d_off.as<const uint64_t>(), d_sizes.as<uint64_t>(), d_flag.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> sizes(3u * (size_t)n);
    uint32_t flag = 0;
    VS_HIP(ctx, hipMemcpyAsync(sizes.data(), d_sizes.ptr(), sizes.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipMemcpyAsync(&flag, d_flag.ptr(), sizeof flag, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    if (flag & 1u) return vs_fail(ctx, VS_E_ARG, "%s: negative count", who);
    InfoPlan plan;
    plan.make(sizes, n);
    VS_HIP(ctx, hipMemcpyAsync(d_row_off.ptr(), plan.row_off.data(), plan.row_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    const unsigned n_buf = plan.n_blocks > 1u ? 2u : plan.n_blocks;
    const uint64_t nm_cap = info_members(plan.cap), out_cap = bgzf ? nm_cap * INFO_MEMBER_CAP : plan.cap;
    if (bgzf && nm_cap > 0x7FFFFFFFull / INFO_MEMBER_CAP) return vs_fail(ctx, VS_E_RANGE, "%s: a row of %llu bytes of text is more than one block holds", who, (unsigned long long)plan.cap);
    Events events;
    for (unsigned b = 0; b < n_buf; b++) {
        VS_HIP(ctx, d_text[b].reserve((size_t)out_cap));  // (BGZF: the packed members of a block)
        VS_HIP(ctx, h_text[b].reserve((size_t)out_cap));
        VS_HIP(ctx, hipEventCreateWithFlags(&events.ev[b], hipEventDisableTiming));
    }
    VsDevBuf d_plain;  // BGZF: the text of the block at hand
    std::vector<uint32_t> mres;
    if (bgzf && n_buf) {
        VS_HIP(ctx, d_plain.reserve((size_t)plan.cap));
        VS_HIP(ctx, d_slots.reserve((size_t)(nm_cap * INFO_MEMBER_CAP)));
        VS_HIP(ctx, d_msize.reserve((size_t)nm_cap * sizeof(uint32_t)));
        VS_HIP(ctx, d_moff.reserve((size_t)nm_cap * sizeof(uint32_t)));
        VS_HIP(ctx, d_mres.reserve(2u * (size_t)nm_cap * sizeof(uint32_t)));
        VS_HIP(ctx, d_tmp.reserve(((size_t)nm_cap / 2048u + 2u) * sizeof(uint64_t)));
        VS_HIP(ctx, d_total.reserve(sizeof(uint64_t)));
        mres.resize(2u * (size_t)nm_cap);
    }
    // block k is formatted (BGZF: and deflated, and packed) and copied into pair k % 2 on the stream; the host then writes
    // block k - 1 out of the other pair
    struct Pending { uint64_t base, bytes; unsigned buf; bool any; } prev = {0, 0, 0, false};
    const auto flush = [&](const Pending &p) -> int {
        VS_HIP(ctx, hipEventSynchronize(events.ev[p.buf]));
        if (const int e = pwrite_all(file.fd, h_text[p.buf].as<const uint8_t>(), p.bytes, p.base))
            return vs_fail(ctx, VS_E_ARG, "write to %s failed: %s", path, strerror(e));
        return VS_OK;
    };
    const auto fail_after_sync = [&](int rc) -> int {
        (void)hipStreamSynchronize(st);  // (the buffers die with the call: nothing may still write them)
        return rc;
    };
    uint32_t k = 0;
    uint64_t file_at = 0, members = 0;
    for (uint32_t i0 = 0; i0 < n;) {
        const uint32_t i1 = block_end(plan.row_off, n, i0, plan.block);
        const uint64_t base = plan.row_off[i0], bytes = plan.row_off[i1] - base;
        if (bytes) {
            const unsigned b = k % 2u;
            uint8_t *text = bgzf ? d_plain.as<uint8_t>() : d_text[b].as<uint8_t>();
            hipLaunchKernelGGL(k_info_format, dim3(i1 - i0), dim3(INFO_TPB), 0, st, src, d_ids.as<const uint8_t>(), d_off.as<const uint64_t>(),
                               d_row_off.as<const uint64_t>(), i0, base, text, bytes, d_flag.as<uint32_t>());
            VS_HIP(ctx, hipGetLastError());
            if (!bgzf) {
                VS_HIP(ctx, hipMemcpyAsync(h_text[b].ptr(), d_text[b].ptr(), (size_t)bytes, hipMemcpyDeviceToHost, st));
                VS_HIP(ctx, hipEventRecord(events.ev[b], st));
                if (prev.any)
                    if (int rc = flush(prev)) return fail_after_sync(rc);
                prev = {base, bytes, b, true};
            } else {
                const uint32_t nm = (uint32_t)info_members(bytes);
                uint64_t packed = 0;
                vs_launch_deflate(st, text, bytes, nm, d_slots.as<uint8_t>(), nm_cap * INFO_MEMBER_CAP, INFO_MEMBER_CAP, INFO_MEMBER_CAP,
                                  d_msize.as<uint32_t>(), d_mres.as<uint32_t>());
                VS_HIP(ctx, hipGetLastError());
                if (int rc = vs_scan_u32(ctx, d_msize.as<const uint32_t>(), d_moff.as<uint32_t>(), nm, d_tmp.as<uint64_t>(), d_total.as<uint64_t>()))
                    return fail_after_sync(rc);
                vs_launch_deflate_pack(st, d_slots.as<const uint8_t>(), INFO_MEMBER_CAP, d_msize.as<const uint32_t>(), d_moff.as<const uint32_t>(), nm,
                                       d_text[b].as<uint8_t>(), out_cap);
                VS_HIP(ctx, hipGetLastError());
                VS_HIP(ctx, hipMemcpyAsync(mres.data(), d_mres.ptr(), 2u * (size_t)nm * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                VS_HIP(ctx, hipMemcpyAsync(&packed, d_total.ptr(), sizeof packed, hipMemcpyDeviceToHost, st));
                if (prev.any)  // (the device works on block k while block k - 1 is written)
                    if (int rc = flush(prev)) return fail_after_sync(rc);
                VS_HIP(ctx, hipStreamSynchronize(st));
                for (uint32_t m = 0; m < nm; m++)
                    if (mres[2u * m] != DEF_OK)
                        return vs_fail(ctx, VS_E_STATE, "%s: member %llu (block %u) ended with status %u", who, (unsigned long long)(members + m), k, mres[2u * m]);
                if (packed > out_cap || packed < 28u * (uint64_t)nm) return vs_fail(ctx, VS_E_STATE, "%s: block %u: %llu bytes in %u members", who, k, (unsigned long long)packed, nm);
                VS_HIP(ctx, hipMemcpyAsync(h_text[b].ptr(), d_text[b].ptr(), (size_t)packed, hipMemcpyDeviceToHost, st));
                VS_HIP(ctx, hipEventRecord(events.ev[b], st));
                prev = {file_at, packed, b, true};
                file_at += packed;
                members += nm;
            }
            k++;
        }
        i0 = i1;
    }
    if (prev.any)
        if (int rc = flush(prev)) return rc;
    VS_HIP(ctx, hipMemcpyAsync(&flag, d_flag.ptr(), sizeof flag, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    if (flag & 2u) return vs_fail(ctx, VS_E_STATE, "%s: the counters changed between the two passes", who);
    res[0] = plan.lines, res[1] = plan.row_off[n], res[2] = k, res[3] = plan.reads, res[4] = members;
    return finish(file_at);
}

// The host twin: the same cells through the same text (vs_info_core.h, and vs_deflate_core.h for BGZF), one thread, host
// pointers, no device.
int info_write_host(vs_ctx *ctx, const char *who, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *counts,
                    const int64_t *wide, const uint8_t *tile_map, const uint32_t *rank, int upper, int dense, bool bgzf, uint64_t res[6]) {
    if (int rc = info_check_args(ctx, who, path, ids, id_off, n, counts, wide, rank)) return rc;
    for (int i = 0; i < 6; i++) res[i] = 0;
    VsInfoSrc src;
    src.counts = counts, src.wide = wide, src.map = counts ? tile_map : nullptr, src.rank = rank;
    src.n = n, src.T = (n + 63u) >> VS_INFO_TILE_SHIFT, src.upper = upper ? 1 : 0, src.dense = dense ? 1 : 0;
    std::vector<uint64_t> sizes(3u * (size_t)n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t li = (uint32_t)(id_off[i + 1] - id_off[i]);
        uint32_t reads = 0;
        for (uint32_t j = vs_info_first_col(src, i); j < n; j++) {
            const int64_t v = vs_info_value(src, i, j, &reads);
            if (v < 0) return vs_fail(ctx, VS_E_ARG, "%s: negative count", who);
            if (vs_info_has_line(src, v)) {
                sizes[3u * (size_t)i]++;
                sizes[3u * (size_t)i + 1u] += vs_info_line_len(li, (uint32_t)(id_off[j + 1] - id_off[j]), (uint64_t)v);
            }
        }
        sizes[3u * (size_t)i + 2u] = reads;
    }
    InfoPlan plan;
    plan.make(sizes, n);
    Fd file;
    file.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (file.fd < 0) return vs_fail(ctx, VS_E_ARG, "cannot open %s for writing: %s", path, strerror(errno));
    std::vector<uint8_t> text((size_t)plan.cap), member(bgzf ? INFO_MEMBER_CAP : 0u);
    uint32_t k = 0;
    uint64_t file_at = 0, members = 0;
    for (uint32_t i0 = 0; i0 < n;) {
        const uint32_t i1 = block_end(plan.row_off, n, i0, plan.block);
        const uint64_t base = plan.row_off[i0], bytes = plan.row_off[i1] - base;
        for (uint32_t i = i0; i < i1 && bytes; i++) {
            const uint32_t li = (uint32_t)(id_off[i + 1] - id_off[i]);
            uint64_t at = plan.row_off[i] - base;
            uint32_t reads = 0;
            for (uint32_t j = vs_info_first_col(src, i); j < n; j++) {
                const int64_t v = vs_info_value(src, i, j, &reads);
                if (!vs_info_has_line(src, v)) continue;
                const uint32_t lj = (uint32_t)(id_off[j + 1] - id_off[j]), len = vs_info_line_len(li, lj, (uint64_t)v);
                if (at + len > plan.row_off[i + 1] - base) return vs_fail(ctx, VS_E_STATE, "%s: the counters changed between the two passes", who);
                vs_info_put_line(text.data() + at, ids + id_off[i], li, ids + id_off[j], lj, (uint64_t)v);
                at += len;
            }
        }
        if (bytes && !bgzf) {
            if (const int e = pwrite_all(file.fd, text.data(), bytes, base)) return vs_fail(ctx, VS_E_ARG, "write to %s failed: %s", path, strerror(e));
            k++;
        } else if (bytes) {
            for (uint64_t at = 0; at < bytes; at += DEF_MAX_TEXT) {
                uint32_t size = 0, kind = 0;
                const uint32_t st = vs_deflate_member_host(text.data() + at, (uint32_t)std::min<uint64_t>(DEF_MAX_TEXT, bytes - at), member.data(),
                                                           INFO_MEMBER_CAP, &size, &kind);
                if (st != DEF_OK) return vs_fail(ctx, VS_E_STATE, "%s: member %llu (block %u) ended with status %u", who, (unsigned long long)members, k, st);
                if (const int e = pwrite_all(file.fd, member.data(), size, file_at)) return vs_fail(ctx, VS_E_ARG, "write to %s failed: %s", path, strerror(e));
                file_at += size;
                members++;
            }
            k++;
        }
        i0 = i1;
    }
    res[0] = plan.lines, res[1] = plan.row_off[n], res[2] = k, res[3] = plan.reads, res[4] = members;
    if (bgzf) {
        if (const int e = pwrite_all(file.fd, vs_bgzf_eof, sizeof vs_bgzf_eof, file_at)) return vs_fail(ctx, VS_E_ARG, "write to %s failed: %s", path, strerror(e));
        res[5] = file_at + sizeof vs_bgzf_eof;
    }
    return VS_OK;
}

}  // namespace

extern "C" int vs_write_info_sparse(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *d_counts,
                                    const int64_t *d_wide, const uint8_t *d_tile_map, const uint32_t *rank, int upper, uint64_t info[4]) {
    uint64_t res[6];
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    const int rc = info_write_device(ctx, "vs_write_info_sparse", path, ids, id_off, n, d_counts, d_wide, d_tile_map, rank, upper, 0, false, res);
    if (rc == VS_OK && info) info[0] = res[0], info[1] = res[1], info[2] = res[2], info[3] = res[3];
    return rc;
}

extern "C" int vs_write_info_sparse_host(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *counts,
                                         const int64_t *wide, const uint8_t *tile_map, const uint32_t *rank, int upper, uint64_t info[4]) {
    uint64_t res[6];
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    const int rc = info_write_host(ctx, "vs_write_info_sparse_host", path, ids, id_off, n, counts, wide, tile_map, rank, upper, 0, false, res);
    if (rc == VS_OK && info) info[0] = res[0], info[1] = res[1], info[2] = res[2], info[3] = res[3];
    return rc;
}

extern "C" int vs_write_info_bgzf(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *d_counts,
                                  const int64_t *d_wide, const uint8_t *d_tile_map, const uint32_t *rank, int upper, int dense, uint64_t info[6]) {
    uint64_t res[6] = {0, 0, 0, 0, 0, 0};
    const int rc = info_write_device(ctx, "vs_write_info_bgzf", path, ids, id_off, n, d_counts, d_wide, d_tile_map, rank, upper, dense, true, res);
    if (info)
        for (int i = 0; i < 6; i++) info[i] = rc == VS_OK ? res[i] : 0;
    return rc;
}

extern "C" int vs_write_info_bgzf_host(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n, const uint32_t *counts,
                                       const int64_t *wide, const uint8_t *tile_map, const uint32_t *rank, int upper, int dense, uint64_t info[6]) {
    uint64_t res[6] = {0, 0, 0, 0, 0, 0};
    const int rc = info_write_host(ctx, "vs_write_info_bgzf_host", path, ids, id_off, n, counts, wide, tile_map, rank, upper, dense, true, res);
    if (info)
        for (int i = 0; i < 6; i++) info[i] = rc == VS_OK ? res[i] : 0;
    return rc;
}

// ---- reader ---------------------------------------------------------------------------------------
// formats.read_pe_text (process_pe_info, IO.py:603-612) on the host threads: lines up to the first empty one, each line
// minus its last character split at ':', the first three fields taken, the count an optionally signed decimal integer;
// then the id filter of the table's builder (a line naming an id that is not in the list is skipped).
namespace {

struct InfoCells {
    std::vector<uint32_t> rows, cols;
    std::vector<int64_t> vals;
    uint64_t lines = 0, skipped = 0, bad_at = UINT64_MAX;
};

// the line txt[lo, hi) (its last character already dropped): 0 a cell, 1 skipped (unknown id), 2 malformed
int parse_line(const uint8_t *txt, uint64_t lo, uint64_t hi, const std::unordered_map<std::string_view, uint32_t> &index, uint32_t *r, uint32_t *c,
               int64_t *val) {
    const uint8_t *p = txt + lo, *e = txt + hi;
    const uint8_t *c1 = (const uint8_t *)memchr(p, ':', (size_t)(e - p));
    if (!c1) return 2;
    const uint8_t *c2 = (const uint8_t *)memchr(c1 + 1, ':', (size_t)(e - c1 - 1));
    if (!c2) return 2;
    const uint8_t *q = c2 + 1;
    const uint8_t *c3 = (const uint8_t *)memchr(q, ':', (size_t)(e - q));
    const uint8_t *qe = c3 ? c3 : e;
    bool minus = false;
    if (q < qe && (*q == '+' || *q == '-')) minus = *q++ == '-';
    if (q == qe) return 2;
    uint64_t mag = 0;
    for (; q < qe; q++) {
        if (*q < '0' || *q > '9') return 2;
        const uint64_t d = (uint64_t)(*q - '0');
        if (mag > (0x8000000000000000ull - d) / 10u) return 2;  // (beyond int64: refused, the tables are int64)
        mag = mag * 10u + d;
    }
    if (!minus && mag > 0x7FFFFFFFFFFFFFFFull) return 2;
    *val = minus ? (int64_t)(0ull - mag) : (int64_t)mag;
    const auto u = index.find(std::string_view((const char *)p, (size_t)(c1 - p)));
    const auto v = index.find(std::string_view((const char *)c1 + 1, (size_t)(c2 - c1 - 1)));
    if (u == index.end() || v == index.end()) return 1;
    *r = u->second, *c = v->second;
    return 0;
}

// every gzip member of p[0, n) inflated behind one another (zlib); false and zlib's words for a corrupt or cut-off stream
bool gunzip_all(const uint8_t *p, uint64_t n, std::vector<uint8_t> &out, std::string &why) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) {
        why = "zlib: inflateInit2 failed";
        return false;
    }
    out.resize((size_t)std::max<uint64_t>(1u << 16, std::min<uint64_t>(n * 4u, 1ull << 30)));
    uint64_t in_at = 0, out_at = 0;
    bool ok = true, ended = false;
    while (ok) {
        if (!z.avail_in && in_at < n) {
            z.next_in = const_cast<Bytef *>(p + in_at);
            z.avail_in = (uInt)std::min<uint64_t>(n - in_at, 1u << 30);
            in_at += z.avail_in;
        }
        if (ended) {
            if (!z.avail_in) break;  // the file ends behind a member
            ended = false;
            if (inflateReset(&z) != Z_OK) ok = false, why = "zlib: inflateReset failed";
            continue;
        }
        if (out_at == out.size()) out.resize(out.size() * 2u);
        z.next_out = out.data() + out_at;
        z.avail_out = (uInt)std::min<uint64_t>(out.size() - out_at, 1u << 30);
        const uInt before = z.avail_out;
        const int rc = inflate(&z, Z_NO_FLUSH);
        out_at += before - z.avail_out;
        if (rc == Z_STREAM_END) ended = true;
        else if (rc == Z_BUF_ERROR && !z.avail_in && in_at >= n) ok = false, why = "gzip stream ends inside a member (unexpected end of file)";
        else if (rc != Z_OK && rc != Z_BUF_ERROR) ok = false, why = std::string("zlib: ") + (z.msg ? z.msg : "error") ;
        else if (rc == Z_OK && !z.avail_in && in_at >= n && z.avail_out) ok = false, why = "gzip stream ends inside a member (unexpected end of file)";
    }
    inflateEnd(&z);
    out.resize((size_t)out_at);
    return ok;
}

}  // namespace

extern "C" int vs_info_parse(const char *path, const uint8_t *names, const uint64_t *name_off, uint32_t n, uint32_t *rows, uint32_t *cols,
                             int64_t *vals, uint64_t cap, uint64_t info[4]) {
    if (!path || !name_off || !info || (n && !names) || (cap && (!rows || !cols || !vals))) return vs_fail(nullptr, VS_E_ARG, "vs_info_parse: bad argument");
    info[0] = info[1] = info[2] = info[3] = 0;
    Fd file;
    file.fd = open(path, O_RDONLY);
    if (file.fd < 0) return vs_fail(nullptr, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
    struct stat sb;
    if (fstat(file.fd, &sb) != 0) return vs_fail(nullptr, VS_E_ARG, "cannot stat %s: %s", path, strerror(errno));
    uint64_t size = (uint64_t)sb.st_size;
    if (!size) return VS_OK;
    void *mp = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, file.fd, 0);
    if (mp == MAP_FAILED) return vs_fail(nullptr, VS_E_OOM, "cannot map %s: %s", path, strerror(errno));
    struct Unmap {
        void *p;
        size_t n;
        ~Unmap() { munmap(p, n); }
    } unmap{mp, (size_t)size};
    const uint8_t *txt = (const uint8_t *)mp;
    std::vector<uint8_t> plain;
    if (size >= 2u && txt[0] == 0x1fu && txt[1] == 0x8bu) {  // gzip, BGZF or not: every member, on the host; then as the plain file
        std::string why;
        if (!gunzip_all(txt, size, plain, why)) return vs_fail(nullptr, VS_E_ARG, "%s: %s", path, why.c_str());
        txt = plain.data(), size = plain.size();
        if (!size) return VS_OK;
    }
    const unsigned T = (unsigned)std::max<uint64_t>(1u, std::min<uint64_t>(vs_host_threads(), size >> 16));
    // a '\r' (universal newlines are Python's) or a byte >= 0x80 (the text decoding is Python's) anywhere: not parsed here
    std::vector<uint32_t> part_flags(T, 0);
    std::vector<std::thread> th;
    const auto run = [&](auto fn) {
        th.clear();
        for (unsigned p = 1; p < T; p++) th.emplace_back(fn, p);
        fn(0u);
        for (auto &t : th) t.join();
    };
    run([&](unsigned p) {
        const uint64_t lo = size * p / T, hi = size * (p + 1) / T;
        uint32_t f = 0;
        if (memchr(txt + lo, '\r', (size_t)(hi - lo))) f |= 1u;
        for (uint64_t x = lo; x < hi && !(f & 2u); x++) f |= txt[x] >= 0x80u ? 2u : 0u;
        part_flags[p] = f;
    });
    for (unsigned p = 0; p < T; p++) info[1] |= part_flags[p];
    if (info[1]) return VS_OK;
    // the text ends in front of the first empty line: a '\n' at the start of the file or right behind another
    uint64_t end = size;
    if (txt[0] == '\n') end = 0;
    else if (const void *q = memmem(txt, (size_t)size, "\n\n", 2)) end = (uint64_t)((const uint8_t *)q - txt) + 1u;
    if (!end) return VS_OK;
    // every thread takes the lines that START in its byte range
    std::vector<InfoCells> part(T);
    std::unordered_map<std::string_view, uint32_t> index;
    if (cap) {
        index.reserve((size_t)n * 2u);
        for (uint32_t i = 0; i < n; i++)  // (a name listed twice keeps its last position, as a dict built in order does)
            index[std::string_view((const char *)names + name_off[i], (size_t)(name_off[i + 1] - name_off[i]))] = i;
    }
    run([&](unsigned p) {
        uint64_t lo = end * p / T;
        const uint64_t hi = end * (p + 1) / T;
        if (lo) {  // first line start at or behind lo
            const void *q = memchr(txt + lo - 1, '\n', (size_t)(end - (lo - 1)));
            lo = q ? (uint64_t)((const uint8_t *)q - txt) + 1u : end;
        }
        InfoCells &out = part[p];
        while (lo < hi && lo < end) {
            const void *q = memchr(txt + lo, '\n', (size_t)(end - lo));
            // (a last line without a newline loses its last character all the same: line[:-1])
            const uint64_t stop = q ? (uint64_t)((const uint8_t *)q - txt) : end - 1u, next = q ? stop + 1u : end;
            out.lines++;
            if (cap) {
                uint32_t r = 0, c = 0;
                int64_t v = 0;
                const int what = parse_line(txt, lo, stop, index, &r, &c, &v);
                if (what == 2) {
                    out.bad_at = lo;
                    return;
                }
                if (what == 1) out.skipped++;
                else out.rows.push_back(r), out.cols.push_back(c), out.vals.push_back(v);
            }
            lo = next;
        }
    });
    uint64_t cells = 0;
    for (unsigned p = 0; p < T; p++) {
        if (part[p].bad_at != UINT64_MAX) {
            const uint64_t at = part[p].bad_at;
            const void *q = memchr(txt + at, '\n', (size_t)(end - at));
            const size_t len = std::min<size_t>(q ? (size_t)((const uint8_t *)q - (txt + at)) : (size_t)(end - at), 60u);
            return vs_fail(nullptr, VS_E_ARG, "%s: malformed line at byte %llu: '%.*s' (expected id:id:count)", path, (unsigned long long)at, (int)len,
                           (const char *)txt + at);
        }
        info[2] += part[p].lines, info[3] += part[p].skipped;
        cells += part[p].rows.size();
    }
    if (!cap) {  // the sizes only: an upper bound on the cells
        info[0] = info[2];
        return VS_OK;
    }
    if (cells > cap) return vs_fail(nullptr, VS_E_RANGE, "vs_info_parse: %llu cells, room for %llu", (unsigned long long)cells, (unsigned long long)cap);
    uint64_t at = 0;
    for (unsigned p = 0; p < T; p++) {
        const size_t m = part[p].rows.size();
        if (!m) continue;
        memcpy(rows + at, part[p].rows.data(), m * sizeof(uint32_t));
        memcpy(cols + at, part[p].cols.data(), m * sizeof(uint32_t));
        memcpy(vals + at, part[p].vals.data(), m * sizeof(int64_t));
        at += m;
    }
    info[0] = cells;
    return VS_OK;
}
