// BGZF members inflated on the device: the blocked gzip that bgzip, htslib and samtools write.  Every member is at most
// 64 KiB in and out, names its own size in its header (the `BC` extra subfield) and its inflated size and CRC32 in its
// trailer, and depends on no other member -- so the members of a chunk are found without inflating anything
// (vs_bgzf_parse) and inflated all at once (k_inflate).
//
// k_inflate: ONE WAVEFRONT PER MEMBER (a workgroup of 64).  The decoder is inf_member of vs_inflate_core.h, the same text
// the host runs in vs_inflate_host.  Its Huffman tables (a 10-bit first-level lookup for literal/length, 8 bits for
// distance, canonical count/symbol arrays behind them for longer codes), the code-length arrays, a 512-byte window of the
// payload and the CRC table live in LDS, about 5.5 KB per wavefront.  The tables are built by the whole wavefront (lane 0
// sorts the symbols, the lanes fill the lookup), the symbol loop runs on wave-uniform state, the bytes of a match and of a
// stored block are copied by all lanes, and CRC32 runs per lane over 64 slices of the output that are combined with the
// x^(8n) mod P multiply of zlib's crc32_combine.
//
// WHERE A MATCH READS ITS SOURCE: the member's own output in global memory; no 32 KiB window per wavefront in LDS, which
// would hold a compute unit to four members in flight.  Why a lane sees the bytes another lane of its wavefront stored a
// few instructions earlier: a wavefront's vector memory instructions are issued in program order as wave-wide operations
// to the one vector L1 of its compute unit, which writes through and serves a later load of the same wavefront after
// the earlier store to the same address -- the hardware does not know lanes apart there, it is the ordering a single lane's
// store-then-load relies on.  The AMDGPU memory model states it as: an acquire/release fence at wavefront scope needs no
// instruction.  What must still be pinned is the compiler, and INF_SYNC (release fence, scheduling barrier, acquire fence,
// all at wavefront scope) does that before every match copy and around every LDS hand-over.  A match never reads what it
// writes itself: a copy with distance < length repeats its first `distance` bytes, all of which precede the match.
//
// A member that fails any check ends with its status word and has written nothing outside [out_off, out_off + ISIZE).
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vs_inflate_core.h"
#include "vs_internal.h"

// ---- the walker (host) -------------------------------------------------------------------------------------------------
// p[0, avail): 0 and *m (in_off relative to p, out_off 0), *member_size when a whole BGZF member starts at p; 1 when what
// is there could still become one ("need more bytes"); 2 when it cannot ("not BGZF").  vs_bgzf_header is its first half:
// the same verdict from the header alone (*header_size up to the payload, *member_size = BSIZE + 1), for a walk that hops
// from header to header without reading a payload.
int vs_bgzf_header(const uint8_t *p, size_t avail, size_t *header_size, size_t *member_size) {
    static const uint8_t magic[4] = {0x1f, 0x8b, 0x08, 0x04};
    for (size_t i = 0; i < 4 && i < avail; i++)
        if (p[i] != magic[i]) return 2;
    if (avail < 12) return 1;
    const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
    if (avail < 12 + xlen) return 1;
    size_t bsize = 0;
    bool found = false;
    for (size_t at = 0; at < xlen;) {
        if (at + 4 > xlen) return 2;
        const uint8_t *q = p + 12 + at;
        const size_t slen = (size_t)q[2] | ((size_t)q[3] << 8);
        if (at + 4 + slen > xlen) return 2;
        if (q[0] == 66 && q[1] == 67 && slen == 2 && !found) {
            bsize = ((size_t)q[4] | ((size_t)q[5] << 8)) + 1u;
            found = true;
        }
        at += 4 + slen;
    }
    if (!found || bsize < 12 + xlen + 8) return 2;
    *header_size = 12 + xlen;
    *member_size = bsize;
    return 0;
}

int vs_bgzf_parse(const uint8_t *p, size_t avail, vs_bgzf_member *m, size_t *member_size) {
    size_t head = 0, bsize = 0;
    if (const int st = vs_bgzf_header(p, avail, &head, &bsize)) return st;
    if (avail < bsize) return 1;
    const uint8_t *t = p + bsize - 8;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (isize > INF_MAX_ISIZE) return 2;
    m->in_off = (uint32_t)head;
    m->in_len = (uint32_t)(bsize - head - 8);  // < 65536
    m->out_off = 0;
    m->isize = isize;
    m->crc = crc;
    *member_size = bsize;
    return 0;
}

// ---- the kernel --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VS_WAVE) k_inflate(const uint8_t *__restrict__ comp, uint64_t comp_size, uint8_t *out, uint64_t out_size,
                                                     const vs_bgzf_member *__restrict__ dir, uint32_t n, uint32_t *__restrict__ status,
                                                     uint32_t *first_bad, uint32_t base, int reversed) {
    __shared__ InfState S;
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= n) return;
    const vs_bgzf_member *e = dir + (reversed ? n - 1u - m : m);  // (the streamed ingest's directory grows downwards)
    const uint32_t in_off = INF_UNI(e->in_off), in_len = INF_UNI(e->in_len), out_off = INF_UNI(e->out_off);
    const uint32_t isize = INF_UNI(e->isize), crc = INF_UNI(e->crc);
    uint32_t st = INF_E_ARG;
    if (isize <= INF_MAX_ISIZE && in_len < 65536u && (uint64_t)in_off + in_len <= comp_size && (uint64_t)out_off + isize <= out_size) {
        uint8_t *o = out + out_off;
        inf_crc_table(&S, lane, VS_WAVE);
        st = inf_member(&S, comp + in_off, in_len, o, isize, lane, VS_WAVE);
        if (st == INF_OK) {
            INF_SYNC();
            uint32_t c = inf_crc_part(&S, o, isize, lane);
#pragma unroll
            for (uint32_t k = VS_WAVE / 2u; k; k >>= 1) c ^= __shfl_xor(c, k);
            if (c != crc) st = INF_E_CRC;
        }
    }
    if (lane == 0) {
        status[m] = st;
        if (st != INF_OK && first_bad) atomicMin(first_bad, base + m);
    }
}

void vs_launch_inflate(hipStream_t st, const uint8_t *comp, uint64_t comp_size, uint8_t *out, uint64_t out_size, const vs_bgzf_member *dir,
                       uint32_t n, uint32_t *status, uint32_t *first_bad, uint32_t base, int reversed) {
    if (n) hipLaunchKernelGGL(k_inflate, dim3(n), dim3(VS_WAVE), 0, st, comp, comp_size, out, out_size, dir, n, status, first_bad, base, reversed);
}

// ---- host form and test aids -------------------------------------------------------------------------------------------
uint32_t vs_inflate_member_host(const uint8_t *pay, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc) {
    if (isize > INF_MAX_ISIZE || len >= 65536u) return INF_E_ARG;
    InfState *S = new InfState();
    inf_crc_table(S, 0, 1);
    uint32_t st = inf_member(S, pay, len, out, isize, 0, 1);
    if (st == INF_OK) {
        uint32_t c = 0;
        for (uint32_t part = 0; part < INF_CRC_PARTS; part++) c ^= inf_crc_part(S, out, isize, part);
        if (c != crc) st = INF_E_CRC;
    }
    delete S;
    return st;
}

// the count of k_inflate_count with one lane: res[0 .. 3] as the kernel writes them
void vs_inflate_count_member_host(const uint8_t *pay, uint32_t len, uint32_t isize, uint32_t crc, uint32_t res[4]) {
    res[0] = INF_E_ARG;
    res[1] = res[2] = res[3] = 0;
    if (isize > INF_MAX_ISIZE || len >= 65536u) return;
    InfState *S = new InfState();
    std::vector<uint8_t> out(isize ? isize : 1u);
    inf_crc_table(S, 0, 1);
    uint32_t st = inf_member(S, pay, len, out.data(), isize, 0, 1);
    if (st == INF_OK) {
        uint32_t c = 0, nl = 0, fl = 0;
        for (uint32_t part = 0; part < INF_CRC_PARTS; part++) c ^= inf_crc_count_part(S, out.data(), isize, part, nl, fl);
        if (c != crc) st = INF_E_CRC;
        else {
            res[1] = nl;
            res[2] = fl;
            res[3] = isize ? out[isize - 1u] : 0u;
        }
    }
    res[0] = st;
    delete S;
}

// ---- the record range of a rank in per-member line counts (host) --------------------------------------------------------------
// counts[0, n): newlines per member of ONE file, in file order; no_final_newline: the file's last byte is no '\n' (its last
// line then counts although no newline ends it, as PE_Inference.py:154 counts it).  Record r is lines 4r .. 4r+3.  For the
// records [first, last): plan[0] = the first member to open, plan[1] = the lines to skip in front of it, plan[2] = one past
// the last member needed.  The first member is the one that holds the newline in front of line 4 * first (member 0, nothing
// skipped, for first == 0): what lies behind that newline cannot be told from counts alone, so a range that starts exactly
// on a member boundary still opens the member before it, only to skip all of it; neighbours share that one member and no
// other.  An empty range opens nothing: {0, 0, 0}.  Returns 1 when the file has fewer than 4 * last lines, else 0.
static int shard_plan(const uint32_t *counts, uint64_t n, int no_final_newline, uint64_t first, uint64_t last, uint64_t plan[3]) {
    plan[0] = plan[1] = plan[2] = 0;
    if (last <= first) return 0;
    const uint64_t line0 = 4u * first, line1 = 4u * last;  // newline number line0 (counted from 1) ends the line in front
    uint64_t before = 0, m = 0;
    if (line0) {
        while (m < n && before + counts[m] < line0) before += counts[m++];
        if (m == n) return 1;
        plan[0] = m;
        plan[1] = line0 - before;
    }
    while (m < n && before + counts[m] < line1) before += counts[m++];
    if (m < n) {
        plan[2] = m + 1u;
        return 0;
    }
    plan[2] = n;  // the last line has no newline: it runs to the end of the file
    return (no_final_newline && before + 1u == line1) ? 0 : 1;
}


extern "C" {

int vs_bgzf_walk(const uint8_t *buf, uint64_t n, uint64_t *members, uint64_t cap, uint64_t info[3]) {
    if ((!buf && n) || !info || (!members && cap)) return vs_fail(nullptr, VS_E_ARG, "vs_bgzf_walk: bad argument");
    uint64_t at = 0, count = 0;
    int state = 0;
    while (at < n) {
        vs_bgzf_member m;
        size_t size = 0;
        state = vs_bgzf_parse(buf + at, (size_t)(n - at), &m, &size);
        if (state) break;
        if (count < cap) {
            members[4 * count + 0] = at + m.in_off;
            members[4 * count + 1] = m.in_len;
            members[4 * count + 2] = m.isize;
            members[4 * count + 3] = m.crc;
        }
        count++;
        at += size;
    }
    info[0] = count;
    info[1] = at;
    info[2] = (uint64_t)state;
    return VS_OK;
}

int vs_inflate_host(const uint8_t *payload, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc, uint32_t *status) {
    if ((!payload && len) || (!out && isize) || !status) return vs_fail(nullptr, VS_E_ARG, "vs_inflate_host: bad argument");
    *status = vs_inflate_member_host(payload, len, out, isize, crc);
    return VS_OK;
}

int vs_inflate_count_host(const uint8_t *payload, uint32_t len, uint32_t isize, uint32_t crc, uint32_t res[4]) {
    if ((!payload && len) || !res) return vs_fail(nullptr, VS_E_ARG, "vs_inflate_count_host: bad argument");
    vs_inflate_count_member_host(payload, len, isize, crc, res);
    return VS_OK;
}

int vs_bgzf_shard_plan(const uint32_t *counts, uint64_t n_members, int no_final_newline, uint64_t first, uint64_t last, uint64_t plan[3]) {
    if ((!counts && n_members) || !plan || first > last || last > (1ull << 60))
        return vs_fail(nullptr, VS_E_ARG, "vs_bgzf_shard_plan: bad argument");
    if (shard_plan(counts, n_members, no_final_newline, first, last, plan))
        return vs_fail(nullptr, VS_E_RANGE, "vs_bgzf_shard_plan: records [%llu, %llu) lie beyond the lines counted", (unsigned long long)first,
                       (unsigned long long)last);
    return VS_OK;
}

int vs_inflate_bgzf(vs_ctx *ctx, const uint8_t *data, uint64_t n, uint8_t *out, uint64_t out_cap, uint32_t guard, uint32_t *status,
                    uint64_t status_cap, uint64_t info[2]) {
    if (!ctx || (!data && n) || !info || n > 0xFFFF0000ull) return vs_fail(ctx, VS_E_ARG, "vs_inflate_bgzf: bad argument");
    std::vector<vs_bgzf_member> dir;
    uint64_t at = 0, total = 0;
    while (at < n) {
        vs_bgzf_member m;
        size_t size = 0;
        if (vs_bgzf_parse(data + at, (size_t)(n - at), &m, &size) != 0)
            return vs_fail(ctx, VS_E_ARG, "vs_inflate_bgzf: no whole BGZF member at byte %llu", (unsigned long long)at);
        m.in_off += (uint32_t)at;
        m.out_off = (uint32_t)total;
        total += (uint64_t)m.isize + guard;
        if (total > 0xFFFF0000ull) return vs_fail(ctx, VS_E_ARG, "vs_inflate_bgzf: more than 4 GiB of output");
        dir.push_back(m);
        at += size;
    }
    info[0] = dir.size();
    info[1] = total;
    if (!out) return VS_OK;  // (the sizes only)
    if (out_cap < total || status_cap < dir.size() || (!status && !dir.empty())) return vs_fail(ctx, VS_E_ARG, "vs_inflate_bgzf: buffers too small");
    if (dir.empty()) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t nm = (uint32_t)dir.size();
    VsDevBuf comp_buf, out_buf, dir_buf, status_buf;
    VS_HIP(ctx, comp_buf.reserve(n + 16u));
    VS_HIP(ctx, out_buf.reserve(total + 16u));
    VS_HIP(ctx, dir_buf.reserve(sizeof(vs_bgzf_member) * nm));
    VS_HIP(ctx, status_buf.reserve(sizeof(uint32_t) * nm));
    uint8_t *d_comp = comp_buf.as<uint8_t>(), *d_out = out_buf.as<uint8_t>();
    vs_bgzf_member *d_dir = dir_buf.as<vs_bgzf_member>();
    uint32_t *d_status = status_buf.as<uint32_t>();
    VS_HIP(ctx, hipMemcpyAsync(d_comp, data, n, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(d_dir, dir.data(), sizeof(vs_bgzf_member) * nm, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(d_out, 0xA5, total + 16u, st));  // (the guard bytes behind every member keep this)
    VS_HIP(ctx, hipMemsetAsync(d_status, 0xFF, sizeof(uint32_t) * nm, st));
    vs_launch_inflate(st, d_comp, n, d_out, total, d_dir, nm, d_status, nullptr, 0, 0);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipMemcpyAsync(status, d_status, sizeof(uint32_t) * nm, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    return VS_OK;
}

}  // extern "C"
