// BGZF members deflated on the device: the other half of vs_inflate.hip.  A text is cut into members of at most 0xFF00
// bytes (bgzip's cut), every member is independent, and k_deflate runs ONE WAVEFRONT PER MEMBER (a workgroup of 64) through
// def_member of vs_deflate_core.h -- the same text vs_deflate_host runs with one lane, and byte for byte the same output.
// What the encoder does, its tie rules and its bounds are written at the head of that file.  Its state (an 11-bit hash
// table of 16-bit positions, the three histograms, code lengths and codes, the code-length builder's two arrays, the
// per-chunk arrays and a 416-byte bit image) is about 9.6 KB of LDS per wavefront; the CRC32 table of the inflate side
// lies in the same bytes while the CRC is taken, before the encoder starts.
//
// A member is written into a slot of its own (the size is not known before it is made), and k_deflate_pack moves the
// members back to back from an exclusive scan of their sizes: only those bytes ever leave the device.
#include <string.h>

#include <vector>

#include "vs_deflate_core.h"
#include "vs_internal.h"

namespace {

// member m = text[m * 0xFF00, ...) -> slots[m * stride, + sizes[m]); res[2 m] = DEF_* status, res[2 m + 1] = DEF_KIND_*
__global__ void __launch_bounds__(VS_WAVE) k_deflate(const uint8_t *__restrict__ text, uint64_t text_bytes, uint32_t n, uint8_t *slots,
                                                     uint64_t slots_bytes, uint32_t stride, uint32_t cap, uint32_t *__restrict__ sizes,
                                                     uint32_t *__restrict__ res) {
    __shared__ DefState S;
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= n) return;
    const uint64_t at = (uint64_t)m * DEF_MAX_TEXT, slot = (uint64_t)m * stride;
    uint32_t st = DEF_E_ARG, size = 0, kind = 0;
    if (at <= text_bytes && cap <= stride && slot + stride <= slots_bytes) {
        const uint64_t left = text_bytes - at;
        const uint32_t len = left < DEF_MAX_TEXT ? (uint32_t)left : DEF_MAX_TEXT;
        st = def_member(&S, text + at, len, slots + slot, cap, lane, VS_WAVE, &size, &kind);
    }
    if (lane == 0) {
        sizes[m] = st == DEF_OK ? size : 0u;
        res[2u * m] = st;
        res[2u * m + 1u] = kind;
    }
}

#define PACK_TPB 256u
__global__ void __launch_bounds__(PACK_TPB) k_deflate_pack(const uint8_t *__restrict__ slots, uint32_t stride, const uint32_t *__restrict__ sizes,
                                                           const uint32_t *__restrict__ offs, uint32_t n, uint8_t *__restrict__ packed,
                                                           uint64_t packed_bytes) {
    const uint32_t m = blockIdx.x;
    if (m >= n) return;
    const uint32_t size = sizes[m], off = offs[m];
    if (size > stride || (uint64_t)off + size > packed_bytes) return;
    const uint8_t *src = slots + (uint64_t)m * stride;
    for (uint32_t i = threadIdx.x; i < size; i += PACK_TPB) packed[off + i] = src[i];
}

}  // namespace

void vs_launch_deflate(hipStream_t st, const uint8_t *text, uint64_t text_bytes, uint32_t n, uint8_t *slots, uint64_t slots_bytes, uint32_t stride,
                       uint32_t cap, uint32_t *sizes, uint32_t *res) {
    if (n) hipLaunchKernelGGL(k_deflate, dim3(n), dim3(VS_WAVE), 0, st, text, text_bytes, n, slots, slots_bytes, stride, cap, sizes, res);
}

void vs_launch_deflate_pack(hipStream_t st, const uint8_t *slots, uint32_t stride, const uint32_t *sizes, const uint32_t *offs, uint32_t n,
                            uint8_t *packed, uint64_t packed_bytes) {
    if (n) hipLaunchKernelGGL(k_deflate_pack, dim3(n), dim3(PACK_TPB), 0, st, slots, stride, sizes, offs, n, packed, packed_bytes);
}

uint32_t vs_deflate_member_host(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *size, uint32_t *kind) {
    DefState *S = new DefState();
    const uint32_t st = def_member(S, text, n, out, cap, 0, 1, size, kind);
    delete S;
    return st;
}

const uint8_t vs_bgzf_eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

extern "C" {

int vs_deflate_host(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *size, uint32_t *kind) {
    if ((!text && n) || (!out && cap) || !size || !kind) return vs_fail(nullptr, VS_E_ARG, "vs_deflate_host: bad argument");
    const uint32_t st = vs_deflate_member_host(text, n, out, cap, size, kind);
    if (st == DEF_E_ARG) return vs_fail(nullptr, VS_E_ARG, "vs_deflate_host: a member takes at most %u bytes of text, not %u", DEF_MAX_TEXT, n);
    if (st == DEF_E_CAP) return vs_fail(nullptr, VS_E_RANGE, "vs_deflate_host: the member does not fit into %u bytes", cap);
    if (st != DEF_OK) return vs_fail(nullptr, VS_E_STATE, "vs_deflate_host: status %u", st);
    return VS_OK;
}

int vs_deflate_bgzf(vs_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t out_cap, uint32_t guard, uint64_t info[5]) {
    if (!ctx || (!text && n) || !out || !info || n > (1ull << 30) || guard > 4096u) return vs_fail(ctx, VS_E_ARG, "vs_deflate_bgzf: bad argument");
    info[0] = info[1] = info[2] = info[3] = info[4] = 0;
    const uint32_t nm = (uint32_t)((n + DEF_MAX_TEXT - 1u) / DEF_MAX_TEXT);
    const uint32_t cap = DEF_MAX_TEXT + DEF_MEMBER_EXTRA, stride = cap + guard;
    uint64_t total = 0;
    if (nm) {
        VS_HIP(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint64_t slots_bytes = (uint64_t)nm * stride;
        VsDevBuf d_text, d_slots, d_sizes, d_offs, d_res, d_tmp, d_total, d_packed;
        VS_HIP(ctx, d_text.reserve((size_t)n));
        VS_HIP(ctx, d_slots.reserve((size_t)slots_bytes));
        VS_HIP(ctx, d_packed.reserve((size_t)nm * cap));
        VS_HIP(ctx, d_sizes.reserve(sizeof(uint32_t) * nm));
        VS_HIP(ctx, d_offs.reserve(sizeof(uint32_t) * nm));
        VS_HIP(ctx, d_res.reserve(2u * sizeof(uint32_t) * nm));
        VS_HIP(ctx, d_tmp.reserve(sizeof(uint64_t) * ((size_t)nm / 2048u + 2u)));
        VS_HIP(ctx, d_total.reserve(sizeof(uint64_t)));
        VS_HIP(ctx, hipMemcpyAsync(d_text.ptr(), text, (size_t)n, hipMemcpyHostToDevice, st));
        VS_HIP(ctx, hipMemsetAsync(d_slots.ptr(), 0xA5, (size_t)slots_bytes, st));
        VS_HIP(ctx, hipMemsetAsync(d_res.ptr(), 0xFF, 2u * sizeof(uint32_t) * nm, st));
        VS_HIP(ctx, hipMemsetAsync(d_sizes.ptr(), 0, sizeof(uint32_t) * nm, st));
        vs_launch_deflate(st, d_text.as<const uint8_t>(), n, nm, d_slots.as<uint8_t>(), slots_bytes, stride, cap, d_sizes.as<uint32_t>(), d_res.as<uint32_t>());
        VS_HIP(ctx, hipGetLastError());
        if (int rc = vs_scan_u32(ctx, d_sizes.as<const uint32_t>(), d_offs.as<uint32_t>(), nm, d_tmp.as<uint64_t>(), d_total.as<uint64_t>())) return rc;
        vs_launch_deflate_pack(st, d_slots.as<const uint8_t>(), stride, d_sizes.as<const uint32_t>(), d_offs.as<const uint32_t>(), nm,
                               d_packed.as<uint8_t>(), (uint64_t)nm * cap);
        VS_HIP(ctx, hipGetLastError());
        std::vector<uint8_t> slots((size_t)slots_bytes);
        std::vector<uint32_t> sizes(nm), res(2u * (size_t)nm);
        VS_HIP(ctx, hipMemcpyAsync(slots.data(), d_slots.ptr(), (size_t)slots_bytes, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipMemcpyAsync(sizes.data(), d_sizes.ptr(), sizeof(uint32_t) * nm, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipMemcpyAsync(res.data(), d_res.ptr(), 2u * sizeof(uint32_t) * nm, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipMemcpyAsync(&total, d_total.ptr(), sizeof total, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        uint64_t sum = 0;
        for (uint32_t m = 0; m < nm; m++) {
            if (res[2u * m] != DEF_OK) return vs_fail(ctx, VS_E_STATE, "vs_deflate_bgzf: member %u ended with status %u", m, res[2u * m]);
            if (sizes[m] > cap || res[2u * m + 1u] > 2u) return vs_fail(ctx, VS_E_STATE, "vs_deflate_bgzf: member %u: size %u, kind %u", m, sizes[m], res[2u * m + 1u]);
            const uint8_t *slot = slots.data() + (size_t)m * stride;
            for (uint32_t i = sizes[m]; i < stride; i++)  // (the guard bytes and whatever of the slot the member did not need)
                if (slot[i] != 0xA5u) return vs_fail(ctx, VS_E_STATE, "vs_deflate_bgzf: member %u of %u bytes wrote byte %u of its slot", m, sizes[m], i);
            info[2u + res[2u * m + 1u]]++;
            sum += sizes[m];
        }
        if (sum != total) return vs_fail(ctx, VS_E_STATE, "vs_deflate_bgzf: the scan gives %llu bytes, the sizes %llu", (unsigned long long)total, (unsigned long long)sum);
        if (out_cap < total + sizeof vs_bgzf_eof) return vs_fail(ctx, VS_E_RANGE, "vs_deflate_bgzf: %llu bytes, room for %llu", (unsigned long long)(total + sizeof vs_bgzf_eof), (unsigned long long)out_cap);
        VS_HIP(ctx, hipMemcpyAsync(out, d_packed.ptr(), (size_t)total, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
    } else if (out_cap < sizeof vs_bgzf_eof) {
        return vs_fail(ctx, VS_E_RANGE, "vs_deflate_bgzf: room for %llu bytes", (unsigned long long)out_cap);
    }
    memcpy(out + total, vs_bgzf_eof, sizeof vs_bgzf_eof);
    info[0] = nm;
    info[1] = total + sizeof vs_bgzf_eof;
    return VS_OK;
}

}  // extern "C"
