// Plain gzip inflated on the device: ONE deflate stream, which has no member directory, decoded by many wavefronts at
// once.  The routines, the symbol space and every bound are those of vs_gzip_core.h (read its head first); this file holds
// the five kernels, the two stages that launch them (gz_front: upload, find, count, chain; gz_back: decode, windows,
// resolve, trailers), and their two callers: the test entry vs_gzip_inflate over a whole buffer (vs_gzip_inflate_host is its
// one-lane twin) and vs_gz_window, which the streamed ingest calls per slot of a plain gzip file and which carries what a
// slot leaves open (vs_gzip_stream.h).
//
//   k_gz_find     one wavefront per span of compressed bytes; its lanes test 64 bit offsets at a time with the cheap filter,
//                 the survivors of a ballot get the full header check by the whole wavefront, one after the other.  With a
//                 granularity the span is that many bytes and the first candidate in it becomes a run start; with
//                 "every candidate" a span is GZ_SPAN_BYTES and hands on up to GZ_SPAN_CAP starts.
//   k_gz_count    one wavefront per start: gz_run<false>.  The host follows the chain (gz_plan_chain) from one download of
//                 the runs' six words each, where it must synchronise anyway to size the buffers.
//   k_gz_decode   one wavefront per chain run: gz_run<true> into the run's own stretch of the symbol buffer.  Launch shape
//                 and LDS state are k_inflate's.  A match reads symbols the same wavefront stored in global memory: the
//                 ordering argument is the one at the head of vs_inflate.hip, INF_SYNC pins the compiler.
//   k_gz_windows  one workgroup walks the chain with the 32 KiB history in LDS and writes the history in front of every run.
//   k_gz_resolve  one wavefront per chain run: symbols to bytes, CRC32 of every segment by 64 slices.
// Every kernel's loops are bounded by the payload, the run count or a run's counted length; no index leaves the buffers
// whose sizes are passed beside them.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "vs_gzip_core.h"
#include "vs_gzip_stream.h"
#include "vs_internal.h"

__global__ void __launch_bounds__(VS_WAVE) k_gz_find(const uint8_t *__restrict__ comp, uint32_t len, uint32_t span, uint32_t spans, uint32_t cap,
                                                     int first_only, uint32_t min_bit, uint32_t *__restrict__ count, uint32_t *__restrict__ list) {
    __shared__ InfState S;
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= spans) return;
    const uint64_t end = (uint64_t)len * 8u, hi = ((uint64_t)s + 1u) * span * 8u;
    const uint32_t n = gz_find_span(&S, comp, len, s * span * 8u, (uint32_t)(hi < end ? hi : end), min_bit, list + (size_t)s * cap, cap, first_only != 0,
                                    lane, VS_WAVE);
    if (lane == 0) count[s] = n;
}

// runs [base, base + grid) of the n starts; span_bits bounds the input of every run but run 0 (0: no bound)
__global__ void __launch_bounds__(VS_WAVE) k_gz_count(const uint8_t *__restrict__ comp, uint32_t len, const uint32_t *__restrict__ starts, uint32_t n,
                                                      GzRun *__restrict__ res, uint32_t base, uint32_t span_bits) {
    __shared__ InfState S;
    const uint32_t i = base + blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    GzRun r;
    gz_run<false>(&S, comp, len, INF_UNI(starts[i]), starts, n, nullptr, GZ_TEXT_MAX, nullptr, 0, r, lane, VS_WAVE, i ? span_bits : 0u);
    if (lane == 0) res[i] = r;
}

__global__ void __launch_bounds__(VS_WAVE) k_gz_decode(const uint8_t *__restrict__ comp, uint32_t len, const uint32_t *__restrict__ starts, uint32_t n,
                                                       const GzChainRun *__restrict__ chain, uint32_t runs, uint16_t *sym, uint64_t sym_size,
                                                       GzMember *mem, uint64_t mem_size, uint32_t *__restrict__ status) {
    __shared__ InfState S;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= runs) return;
    const uint32_t start = INF_UNI(chain[c].start_bit), off = INF_UNI(chain[c].off), want = INF_UNI(chain[c].len);
    const uint32_t mem_off = INF_UNI(chain[c].mem_off), nmem = INF_UNI(chain[c].nmem);
    uint32_t st = INF_E_ARG;
    if ((uint64_t)off + want <= sym_size && (uint64_t)mem_off + nmem <= mem_size) {
        GzRun r;
        gz_run<true>(&S, comp, len, start, starts, n, sym + off, want, mem + mem_off, nmem, r, lane, VS_WAVE);  // (no span: a chain run)
        st = r.status != INF_OK ? r.status : (r.out_len != want || r.nmem != nmem) ? (uint32_t)INF_E_OUT_SHORT : (uint32_t)INF_OK;
    }
    if (lane == 0) status[c] = st;
}

#define GZ_WIN_THREADS 1024u
__global__ void __launch_bounds__(GZ_WIN_THREADS) k_gz_windows(const GzChainRun *__restrict__ chain, uint32_t runs, const uint16_t *__restrict__ sym,
                                                                uint64_t sym_size, uint8_t *__restrict__ hist, const uint8_t *first, uint8_t *last) {
    // first (may be NULL: zeros): the 32 KiB in front of run 0; last (may be NULL, may be first): those behind the last run
    __shared__ uint8_t H[GZ_HIST];
    const uint32_t t = threadIdx.x;
    constexpr uint32_t PER = GZ_HIST / GZ_WIN_THREADS;
    for (uint32_t j = 0; j < PER; j++) H[t + GZ_WIN_THREADS * j] = first ? first[t + GZ_WIN_THREADS * j] : (uint8_t)0;
    __syncthreads();
    for (uint32_t c = 0; c < runs; c++) {
        const uint32_t off = chain[c].off, len = chain[c].len;
        if ((uint64_t)off + len > sym_size) break;  // (uniform; k_gz_decode has reported the run)
        uint8_t v[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            const uint32_t k = t + GZ_WIN_THREADS * j;
            hist[(size_t)c * GZ_HIST + k] = H[k];
            v[j] = gz_window_byte(H, sym + off, len, k);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) H[t + GZ_WIN_THREADS * j] = v[j];
        __syncthreads();
    }
    if (last)
        for (uint32_t j = 0; j < PER; j++) last[t + GZ_WIN_THREADS * j] = H[t + GZ_WIN_THREADS * j];
}

__global__ void __launch_bounds__(VS_WAVE) k_gz_resolve(const GzChainRun *__restrict__ chain, uint32_t runs, const uint16_t *__restrict__ sym,
                                                        uint64_t sym_size, const uint8_t *__restrict__ hist, uint8_t *out, const GzMember *__restrict__ mem,
                                                        uint64_t mem_size, uint32_t *__restrict__ seg_crc, uint32_t *__restrict__ status) {
    __shared__ InfState S;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= runs) return;
    const uint32_t off = INF_UNI(chain[c].off), len = INF_UNI(chain[c].len), mem_off = INF_UNI(chain[c].mem_off), nmem = INF_UNI(chain[c].nmem);
    uint32_t st = INF_E_ARG;
    if ((uint64_t)off + len <= sym_size && (uint64_t)mem_off + nmem <= mem_size) {
        inf_crc_table(&S, lane, VS_WAVE);
        const uint32_t bad = gz_resolve_bytes(sym + off, hist + (size_t)c * GZ_HIST, INF_UNI(chain[c].hist_valid), out + off, len, lane, VS_WAVE);
        st = GZ_BALLOT(bad != 0) ? (uint32_t)INF_E_FAR : (uint32_t)INF_OK;
        INF_SYNC();
        for (uint32_t k = 0; k <= nmem; k++) {
            uint32_t lo, hi;
            gz_segment(mem + mem_off, nmem, len, k, lo, hi);
            uint32_t crc = inf_crc_part(&S, out + off + lo, hi - lo, lane);
#pragma unroll
            for (uint32_t x = VS_WAVE / 2u; x; x >>= 1) crc ^= __shfl_xor(crc, x);
            if (lane == 0) seg_crc[mem_off + c + k] = crc;
        }
    }
    if (lane == 0) status[c] = st;
}

static void put_info(uint64_t info[9], const GzInfo &g) {
    info[0] = g.candidates, info[1] = g.selected, info[2] = g.chain_runs, info[3] = g.dropped;
    info[4] = g.members, info[5] = g.status, info[6] = g.bad_run, info[7] = g.text, info[8] = g.recounted;
}

// upload, find, count and the chain of data[0, len) from the known start start0 (valid: hist_valid of that run)
static int gz_front(vs_ctx *ctx, hipStream_t st, GzDev &d, const uint8_t *data, uint32_t len, uint32_t gran, uint32_t start0, uint32_t valid,
                    uint32_t text_cap, std::vector<uint32_t> &starts, GzPlan &P, uint64_t *candidates, uint64_t *recounted) {
    const uint32_t span = gran ? gran : GZ_SPAN_BYTES, cap = gran ? 1u : GZ_SPAN_CAP, spans = (len + span - 1u) / span;
    VS_HIP(ctx, d.comp.reserve((size_t)len + 16u, (size_t)len + len / 4u + 16u));
    VS_HIP(ctx, d.count.reserve(sizeof(uint32_t) * spans, sizeof(uint32_t) * (spans + spans / 4u)));
    VS_HIP(ctx, d.list.reserve(sizeof(uint32_t) * (size_t)spans * cap, sizeof(uint32_t) * ((size_t)spans + spans / 4u) * cap));
    VS_HIP(ctx, hipMemcpyAsync(d.comp.ptr(), data, len, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(d.count.ptr(), 0, sizeof(uint32_t) * spans, st));
    VS_HIP(ctx, hipMemsetAsync(d.list.ptr(), 0, sizeof(uint32_t) * (size_t)spans * cap, st));
    hipLaunchKernelGGL(k_gz_find, dim3(spans), dim3(VS_WAVE), 0, st, d.comp.as<uint8_t>(), len, span, spans, cap, gran != 0 ? 1 : 0, start0 + 1u,
                       d.count.as<uint32_t>(), d.list.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> count(spans), list((size_t)spans * cap);
    VS_HIP(ctx, hipMemcpyAsync(count.data(), d.count.ptr(), sizeof(uint32_t) * spans, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipMemcpyAsync(list.data(), d.list.ptr(), sizeof(uint32_t) * list.size(), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    gz_collect_starts(start0, count.data(), list.data(), spans, cap, starts, *candidates);
    const uint32_t ns = (uint32_t)starts.size();
    VS_HIP(ctx, d.starts.reserve(sizeof(uint32_t) * ns, sizeof(uint32_t) * (ns + ns / 4u)));
    VS_HIP(ctx, d.res.reserve(sizeof(GzRun) * ns, sizeof(GzRun) * (ns + ns / 4u)));
    VS_HIP(ctx, hipMemcpyAsync(d.starts.ptr(), starts.data(), sizeof(uint32_t) * ns, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(d.res.ptr(), 0xFF, sizeof(GzRun) * ns, st));
    hipLaunchKernelGGL(k_gz_count, dim3(ns), dim3(VS_WAVE), 0, st, d.comp.as<uint8_t>(), len, d.starts.as<uint32_t>(), ns, d.res.as<GzRun>(), 0u, gz_span_bits(span));
    VS_HIP(ctx, hipGetLastError());
    std::vector<GzRun> res(ns);
    VS_HIP(ctx, hipMemcpyAsync(res.data(), d.res.ptr(), sizeof(GzRun) * ns, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    gz_plan_chain(starts, res.data(), P, valid, text_cap);
    while (P.status == GZ_E_SPAN) {  // the chain reaches a run that hit its span: that one again, unbounded (at most once per run)
        const uint32_t i = (uint32_t)gz_start_index(starts, P.next_bit);
        hipLaunchKernelGGL(k_gz_count, dim3(1), dim3(VS_WAVE), 0, st, d.comp.as<uint8_t>(), len, d.starts.as<uint32_t>(), ns, d.res.as<GzRun>(), i, 0u);
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(&res[i], d.res.as<GzRun>() + i, sizeof(GzRun), hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        ++*recounted;
        gz_plan_chain(starts, res.data(), P, valid, text_cap);
    }
    return VS_OK;
}

// decode, windows, resolve of P.chain (not empty) into d_out[0, P.text), the trailers against crc / bytes: *status, *bad_run
static int gz_back(vs_ctx *ctx, hipStream_t st, GzDev &d, uint32_t len, uint32_t ns, const GzPlan &P, uint8_t *d_out, const uint8_t *first,
                   uint8_t *last, uint32_t &crc, uint64_t &bytes, uint32_t *status_out, uint32_t *bad_run) {
    const uint32_t runs = (uint32_t)P.chain.size();
    const uint64_t nseg = P.members + runs;
    VS_HIP(ctx, d.chain.reserve(sizeof(GzChainRun) * runs, sizeof(GzChainRun) * (runs + runs / 4u)));
    VS_HIP(ctx, d.sym.reserve(sizeof(uint16_t) * (P.text + 1u), sizeof(uint16_t) * (P.text + P.text / 4u + 1u)));
    VS_HIP(ctx, d.mem.reserve(sizeof(GzMember) * (P.members + 1u), sizeof(GzMember) * (P.members + P.members / 4u + 1u)));
    VS_HIP(ctx, d.hist.reserve((size_t)GZ_HIST * runs, (size_t)GZ_HIST * (runs + runs / 4u)));
    VS_HIP(ctx, d.seg.reserve(sizeof(uint32_t) * nseg, sizeof(uint32_t) * (nseg + nseg / 4u)));
    VS_HIP(ctx, d.status.reserve(sizeof(uint32_t) * 2u * runs, sizeof(uint32_t) * 2u * (runs + runs / 4u)));
    uint32_t *d_status = d.status.as<uint32_t>();
    VS_HIP(ctx, hipMemcpyAsync(d.chain.ptr(), P.chain.data(), sizeof(GzChainRun) * runs, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(d.mem.ptr(), 0, sizeof(GzMember) * (P.members + 1u), st));
    VS_HIP(ctx, hipMemsetAsync(d.seg.ptr(), 0, sizeof(uint32_t) * nseg, st));
    VS_HIP(ctx, hipMemsetAsync(d_status, 0xFF, sizeof(uint32_t) * 2u * runs, st));
    hipLaunchKernelGGL(k_gz_decode, dim3(runs), dim3(VS_WAVE), 0, st, d.comp.as<uint8_t>(), len, d.starts.as<uint32_t>(), ns, d.chain.as<GzChainRun>(), runs,
                       d.sym.as<uint16_t>(), P.text, d.mem.as<GzMember>(), P.members, d_status);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(GZ_WIN_THREADS), 0, st, d.chain.as<GzChainRun>(), runs, d.sym.as<uint16_t>(), P.text, d.hist.as<uint8_t>(),
                       first, last);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gz_resolve, dim3(runs), dim3(VS_WAVE), 0, st, d.chain.as<GzChainRun>(), runs, d.sym.as<uint16_t>(), P.text, d.hist.as<uint8_t>(), d_out,
                       d.mem.as<GzMember>(), P.members, d.seg.as<uint32_t>(), d_status + runs);
    VS_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> status(2u * runs), seg(nseg);
    std::vector<GzMember> mem(P.members + 1u);
    VS_HIP(ctx, hipMemcpyAsync(status.data(), d_status, sizeof(uint32_t) * 2u * runs, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipMemcpyAsync(seg.data(), d.seg.ptr(), sizeof(uint32_t) * nseg, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipMemcpyAsync(mem.data(), d.mem.ptr(), sizeof(GzMember) * (P.members + 1u), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    *status_out = INF_OK;
    *bad_run = 0;
    for (uint32_t c = 0; c < runs && *status_out == INF_OK; c++) {  // the first failing run, decode before resolve as on one lane
        *status_out = status[c] != INF_OK ? status[c] : status[runs + c];
        *bad_run = *status_out != INF_OK ? c : 0;
    }
    if (*status_out == INF_OK) *status_out = gz_check_members(P, mem.data(), seg.data(), crc, bytes);
    return VS_OK;
}

const char *vs_gz_status_name(uint32_t status) {
    static const char *const names[] = {"INF_OK", "INF_E_BTYPE", "INF_E_STORED", "INF_E_OVERSUB", "INF_E_INCOMPLETE", "INF_E_LITLEN", "INF_E_DIST",
                                        "INF_E_FAR", "INF_E_INPUT", "INF_E_OUT_OVER", "INF_E_OUT_SHORT", "INF_E_CRC", "INF_E_LENGTHS",
                                        "INF_E_TRAILING", "INF_E_ARG", "GZ_E_HEADER", "GZ_E_ISIZE", "GZ_E_SPAN"};
    return status < sizeof names / sizeof names[0] ? names[status] : "?";
}

int vs_gz_window(vs_ctx *ctx, hipStream_t st, GzStream &g, const uint8_t *data, size_t n, bool last, const std::function<int(size_t, uint8_t **)> &room,
                 size_t *text, uint32_t *status) {
    *text = 0;
    *status = INF_OK;
    g.more = false;
    g.last_seen = g.last_seen || last;
    if (n) g.pend.insert(g.pend.end(), data, data + n);
    if (g.pend.size() > GZ_MAX_BYTES)  // (pend grows past a slot only while its first run has not ended)
        return vs_fail(ctx, VS_E_RANGE, "a deflate run of more than %u compressed bytes: leave the device gzip switch out for this input", GZ_MAX_BYTES);
    if (g.at_member) {
        if (g.pend.empty()) return VS_OK;  // (the end of the file behind a trailer, or more to come)
        uint32_t start0 = 0;
        const uint32_t hs = gz_first_header(g.pend.data(), g.pend.size(), &start0);
        if (hs == INF_E_INPUT && !last) return VS_OK;  // (the header is not all here yet)
        if (hs != INF_OK) {
            *status = hs;
            return VS_OK;
        }
        g.at_member = false;
        g.bit = start0;
        g.valid = 0;
    }
    const uint32_t len = (uint32_t)g.pend.size();
    std::vector<uint32_t> starts;
    GzPlan P;
    uint64_t candidates = 0;
    const uint32_t text_cap = g.text_cap < GZ_TEXT_MAX ? g.text_cap : GZ_TEXT_MAX;
    if (int rc = gz_front(ctx, st, g.dev, g.pend.data(), len, GZ_STREAM_GRAN, g.bit, g.valid, text_cap, starts, P, &candidates, &g.recounted)) return rc;
    if (P.status == INF_E_OUT_OVER && P.chain.empty())  // (the plan caps a chain in front of such a run: this one is the first)
        return vs_fail(ctx, VS_E_RANGE, "a deflate run of more than %u bytes of text: leave the device gzip switch out for this input", text_cap);
    const bool cut = P.status == INF_E_INPUT && !last;  // the piece ended inside a run: that run waits for more bytes
    if (P.status != INF_OK && !cut) {
        *status = P.status;
        return VS_OK;
    }
    const bool ended = P.status == INF_OK && !P.capped;  // (on GZ_END: behind a trailer with no byte left)
    if (P.chain.empty()) return VS_OK;  // (cut inside the first run: more bytes are needed; pend keeps what there is)
    g.more = P.capped;  // the longest chain prefix that fits is decoded now, the rest stays compressed for the next round
    uint8_t *d_out = nullptr;
    if (int rc = room((size_t)P.text, &d_out)) return rc;
    VS_HIP(ctx, g.hist0.reserve(GZ_HIST));
    if (g.windows == 0) VS_HIP(ctx, hipMemsetAsync(g.hist0.ptr(), 0, GZ_HIST, st));
    uint32_t bad_run = 0;
    if (int rc = gz_back(ctx, st, g.dev, len, (uint32_t)starts.size(), P, d_out, g.hist0.as<uint8_t>(), g.hist0.as<uint8_t>(), g.crc, g.bytes, status, &bad_run))
        return rc;
    if (*status != INF_OK) return VS_OK;
    g.windows++;
    g.runs += P.chain.size();
    // (dropped: the starts in front of where the chain stopped that are not of it; those behind are the next round's)
    g.dropped += (ended ? starts.size() : (size_t)(std::lower_bound(starts.begin(), starts.end(), P.next_bit) - starts.begin())) - P.chain.size();
    g.members += P.members;
    g.text += P.text;
    *text = (size_t)P.text;
    if (ended) {
        g.pend.clear();
        g.at_member = true;
        g.bit = 0;
    } else {
        g.pend.erase(g.pend.begin(), g.pend.begin() + (P.next_bit >> 3));
        g.bit = P.next_bit & 7u;
    }
    g.valid = P.valid_end;
    return VS_OK;
}

extern "C" {

int vs_gzip_inflate_host(const uint8_t *data, uint64_t n, uint32_t gran, uint8_t *out, uint64_t out_cap, uint64_t info[9]) {
    if ((!data && n) || !info || n > GZ_MAX_BYTES || (gran && gran < 16u)) return vs_fail(nullptr, VS_E_ARG, "vs_gzip_inflate_host: bad argument");
    std::vector<uint8_t> text;
    GzInfo g;
    gz_inflate_one_lane(data, n, gran, text, g);
    put_info(info, g);
    if (!out) return VS_OK;
    if (out_cap < text.size()) return vs_fail(nullptr, VS_E_ARG, "vs_gzip_inflate_host: buffer too small");
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return VS_OK;
}

int vs_gzip_inflate(vs_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t gran, uint8_t *out, uint64_t out_cap, uint32_t guard, uint64_t info[9]) {
    if (!ctx || (!data && n) || !info || n > GZ_MAX_BYTES || (gran && gran < 16u)) return vs_fail(ctx, VS_E_ARG, "vs_gzip_inflate: bad argument");
    GzInfo g;
    uint32_t start0 = 0;
    g.status = gz_first_header(data, n, &start0);
    put_info(info, g);
    if (g.status != INF_OK) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GzDev d;
    std::vector<uint32_t> starts;
    GzPlan P;
    if (int rc = gz_front(ctx, st, d, data, (uint32_t)n, gran, start0, 0, GZ_TEXT_MAX, starts, P, &g.candidates, &g.recounted)) return rc;
    if (P.capped) P.status = INF_E_OUT_OVER;  // (a whole buffer is delivered whole or not at all)
    g.selected = starts.size() - 1u;
    g.chain_runs = P.chain.size();
    g.dropped = starts.size() - P.chain.size();
    g.members = P.members;
    g.status = P.status;
    g.bad_run = P.bad_run;
    g.text = P.status == INF_OK ? P.text : 0;
    put_info(info, g);
    if (!out || P.status != INF_OK) return VS_OK;  // (the sizes only, or nothing to deliver)
    if (out_cap < P.text + guard) return vs_fail(ctx, VS_E_ARG, "vs_gzip_inflate: buffer too small");
    VsDevBuf out_buf;
    VS_HIP(ctx, out_buf.reserve(P.text + guard + 1u));
    VS_HIP(ctx, hipMemsetAsync(out_buf.ptr(), 0xA5, P.text + guard + 1u, st));  // (the guard bytes behind the text keep this)
    uint32_t crc = 0, status = 0, bad_run = 0;
    uint64_t bytes = 0;
    if (int rc = gz_back(ctx, st, d, (uint32_t)n, (uint32_t)starts.size(), P, out_buf.as<uint8_t>(), nullptr, nullptr, crc, bytes, &status, &bad_run)) return rc;
    g.status = status;
    g.bad_run = bad_run;
    if (g.status != INF_OK) g.text = 0;
    else if (P.text + guard) VS_HIP(ctx, hipMemcpy(out, out_buf.ptr(), P.text + guard, hipMemcpyDeviceToHost));
    put_info(info, g);
    return VS_OK;
}

}  // extern "C"
