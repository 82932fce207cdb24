// pe_info / st_info read where the link table lives (vs_links_from_info): the text of both files, inflated on the device when
// it is whole BGZF (k_inflate, vs_inflate.hip), is scanned and parsed in windows by the two kernels below and added straight
// into the table.  The rule of a line, the name lookup and the walk over the windows are vs_info_read_core.h, shared with the
// host twin vs_info_read_host at the end of this file.
//
//   k_info_scan      one pass over a window: every lane takes 16 bytes with one aligned dwordx4 load plus the byte in front;
//                    the '\r' / >= 0x80 flags, the newlines, the first empty line and the last '\n' are reduced per
//                    wavefront (ballot, DPP scans) and leave through at most four atomics per wavefront.  The host reads
//                    the four words back and decides in front of which position a line must start to be parsed (ir_limit).
//   k_info_parse     a workgroup stages a tile of 4096 bytes plus 256 of overhang in LDS, compacts the tile's line starts
//                    into an LDS list (16 bytes per lane, prefix count over the workgroup), then ONE LANE PER LINE parses out
//                    of LDS; a line that runs past the overhang is read from global memory.  DENSE: a non-zero count is added
//                    to P0[r][c] and, off the diagonal, to P0[c][r] by 64-bit atomic adds (int64 adds commute: the argument
//                    k_links_scatter makes).  CSR route: the non-zero cells are appended to a device list through a
//                    wavefront-aggregated counter and downloaded per window for the host's CSR build.
//
// Precedence of outcomes, as vs_info_parse has it: a corrupt gzip stream, then a '\r' or a byte >= 0x80 anywhere in the file
// (Python's to read), then the first malformed line.  So every member is inflated and every byte scanned even behind the end
// of the text.  A file with an error, a line longer than a window, or a gzip file that is not whole BGZF goes to
// vs_info_parse, which words the error.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <vector>

#include "vs_info_read_core.h"
#include "vs_inflate_core.h"
#include "vs_internal.h"

namespace {

#define IR_TPB 256u
#define IR_TILE 4096u   // text bytes per workgroup step: 16 per lane
#define IR_OVER 256u    // staged behind the tile for the lines that start in it
#define IR_MAX_STARTS (IR_TILE / 2u)  // (two line starts are never adjacent in front of the empty line)
#define IR_WINDOW_DEFAULT (256u << 20)
#define IR_WINDOW_MAX (1u << 30)

// the words of a window on the device, zeroed before every window; the two minima are held as maxima of the complement so
// that zero means "none"
enum { IRC_FLAGS = 0, IRC_NEWLINES, IRC_EMPTY_INV, IRC_NL_END, IRC_LINES, IRC_SKIPPED, IRC_BAD_INV, IRC_CELLS, IRC_WORDS };

// txt[0, size) in a buffer whose capacity is a multiple of 16 bytes and 16-byte aligned
__global__ void __launch_bounds__(IR_TPB) k_info_scan(const uint8_t *__restrict__ txt, uint32_t size, uint32_t *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x % VS_WAVE;
    uint32_t flags = 0, newlines = 0, empty_inv = 0, nl_end = 0;
    const uint32_t chunks = (size + 15u) / 16u;
    for (uint32_t i = blockIdx.x * IR_TPB + threadIdx.x; i < chunks; i += gridDim.x * IR_TPB) {
        const uint4 v = reinterpret_cast<const uint4 *>(txt)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t prev = i ? txt[16u * i - 1u] : (uint32_t)'\n';
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t x = 16u * i + k, b = (w[k / 4u] >> (8u * (k % 4u))) & 0xFFu;
            if (x < size) {
                flags |= (b == '\r' ? 1u : 0u) | (b >= 0x80u ? 2u : 0u);
                if (b == '\n') {
                    newlines++;
                    nl_end = x + 1u;
                    if (prev == '\n' && !empty_inv) empty_inv = ~x;  // (ascending in a lane: the first is its smallest)
                }
            }
            prev = b;
        }
    }
    const bool cr = __ballot((flags & 1u) != 0u) != 0ull, high = __ballot((flags & 2u) != 0u) != 0ull;
    newlines = vs_wave_scan_add(newlines);
    empty_inv = vs_wave_scan_max(empty_inv);
    nl_end = vs_wave_scan_max(nl_end);
    if (lane == VS_WAVE - 1u) {  // (the scans end in the last lane)
        if (cr || high) atomicOr(&ctr[IRC_FLAGS], (cr ? 1u : 0u) | (high ? 2u : 0u));
        if (newlines) atomicAdd(&ctr[IRC_NEWLINES], newlines);
        if (empty_inv) atomicMax(&ctr[IRC_EMPTY_INV], empty_inv);
        if (nl_end) atomicMax(&ctr[IRC_NL_END], nl_end);
    }
}

// a text byte for a lane of k_info_parse: out of the staged tile, else from global memory, never outside [0, size)
struct IrTileReader {
    const uint8_t *lds, *txt;
    uint32_t t0, lds_bytes, size;
    __device__ uint8_t operator()(uint64_t x) const {
        if (x >= size) return 0;
        const uint32_t o = (uint32_t)x - t0;
        return o < lds_bytes ? lds[o] : txt[x];
    }
};

// The lines of txt[0, size) that start in front of `limit` (<= size; capacity as for k_info_scan: `cap` bytes, a multiple of 16).
template <bool DENSE>
__global__ void __launch_bounds__(IR_TPB) k_info_parse(const uint8_t *__restrict__ txt, uint32_t size, uint32_t cap, uint32_t limit, const IrNames nm,
                                                       uint32_t n, int64_t *__restrict__ p0, uint32_t *__restrict__ rows, uint32_t *__restrict__ cols,
                                                       int64_t *__restrict__ vals, uint32_t list_cap, uint32_t *__restrict__ ctr) {
    __shared__ uint4 s_txt4[(IR_TILE + IR_OVER) / 16u];
    __shared__ uint16_t s_start[IR_MAX_STARTS];
    __shared__ uint32_t s_wave[IR_TPB / VS_WAVE];
    const uint8_t *s_txt = reinterpret_cast<const uint8_t *>(s_txt4);
    const uint32_t tid = threadIdx.x, lane = tid % VS_WAVE, wave = tid / VS_WAVE, c = 16u * tid;
    const uint32_t tiles = (limit + IR_TILE - 1u) / IR_TILE;
    uint32_t lines = 0, skipped = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t t0 = t * IR_TILE;
        __syncthreads();  // (the tile before is parsed)
        {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((uint64_t)t0 + c + 16u <= cap) v = *reinterpret_cast<const uint4 *>(txt + t0 + c);
            s_txt4[tid] = v;
            if (tid < IR_OVER / 16u) {
                uint4 o = make_uint4(0u, 0u, 0u, 0u);
                if ((uint64_t)t0 + IR_TILE + c + 16u <= cap) o = *reinterpret_cast<const uint4 *>(txt + t0 + IR_TILE + c);
                s_txt4[IR_TILE / 16u + tid] = o;
            }
        }
        __syncthreads();
        // the line starts among my 16 bytes: a position in front of the limit whose byte in front is a '\n'
        uint32_t mask = 0;
        uint32_t prev = tid ? s_txt[c - 1u] : (t0 ? txt[t0 - 1u] : (uint32_t)'\n');
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            if (t0 + c + k < limit && prev == '\n') mask |= 1u << k;
            prev = s_txt[c + k];
        }
        const uint32_t cnt = __popc(mask), incl = vs_wave_scan_add(cnt);
        if (lane == VS_WAVE - 1u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < IR_TPB / VS_WAVE; w++) {
            const uint32_t x = s_wave[w];
            before += w < wave ? x : 0u;
            total += x;
        }
        uint32_t at = before + incl - cnt;
        for (uint32_t m = mask; m; m &= m - 1u, at++)
            if (at < IR_MAX_STARTS) s_start[at] = (uint16_t)(c + (uint32_t)__ffs((int)m) - 1u);
        __syncthreads();
        total = min(total, IR_MAX_STARTS);
        if (tid == 0) lines += total;
        const IrTileReader rd = {s_txt, txt, t0, IR_TILE + IR_OVER, size};
        for (uint32_t i0 = 0; i0 < total; i0 += IR_TPB) {  // (the same trips for every lane: the ballot below takes all of a wavefront)
            const uint32_t i = i0 + tid;
            bool has = false;
            uint32_t r = 0, cc = 0;
            int64_t val = 0;
            if (i < total) {
                const uint32_t p = t0 + s_start[i];
                const uint32_t stop = ir_line_stop(rd, p, size);
                const int what = ir_parse_line(nm, rd, p, stop, &r, &cc, &val);
                if (what == IR_MALFORMED) atomicMax(&ctr[IRC_BAD_INV], ~p);
                else if (what == IR_SKIPPED) skipped++;
                else has = val != 0 && r < n && cc < n;
            }
            if (DENSE) {
                if (has) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&p0[(uint64_t)r * n + cc]), (unsigned long long)val);
                    if (r != cc) atomicAdd(reinterpret_cast<unsigned long long *>(&p0[(uint64_t)cc * n + r]), (unsigned long long)val);
                }
            } else {
                const unsigned long long m = __ballot(has);
                if (m) {  // one atomic per wavefront: its first lane with a cell reserves for all
                    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
                    uint32_t first = 0;
                    if (lane == leader) first = atomicAdd(&ctr[IRC_CELLS], (uint32_t)__popcll(m));
                    first = __shfl(first, (int)leader);
                    const uint32_t slot = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (has && slot < list_cap) rows[slot] = r, cols[slot] = cc, vals[slot] = val;
                }
            }
        }
    }
    skipped = vs_wave_scan_add(skipped);
    if (lane == VS_WAVE - 1u && skipped) atomicAdd(&ctr[IRC_SKIPPED], skipped);
    if (tid == 0 && lines) atomicAdd(&ctr[IRC_LINES], lines);
}

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};
struct Map {
    void *p = MAP_FAILED;
    size_t n = 0;
    ~Map() { if (p != MAP_FAILED) munmap(p, n); }
};

uint32_t clamp_window(uint64_t window_bytes) {
    if (!window_bytes) return IR_WINDOW_DEFAULT;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(window_bytes, 16u), IR_WINDOW_MAX);
}

// the name table of a call, on the host: false when an offset runs backwards
bool build_names(const uint64_t *name_off, uint32_t n, const uint8_t *names, std::vector<uint64_t> &off0, std::vector<IrSlot> &table, uint32_t *bits) {
    off0.assign((size_t)n + 1u, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (name_off[i + 1] < name_off[i]) return false;
        off0[i + 1] = name_off[i + 1] - name_off[0];
    }
    *bits = ir_table_bits(n);
    table.assign((size_t)1u << *bits, IrSlot{0u, IR_EMPTY});
    for (uint32_t i = 0; i < n; i++)
        if (!ir_table_insert(table.data(), *bits, names + name_off[0], off0.data(), off0[n], i)) return false;
    return true;
}

enum { IR_ROUTE_NONE = 0, IR_ROUTE_BGZF = 1, IR_ROUTE_PLAIN = 2, IR_ROUTE_HOST = 3 };
enum { IRO_OK = 0, IRO_PYTHON = 1, IRO_HOST = 2 };  // what became of a file on the device route (IRO_HOST: hand it to vs_info_parse)
// info words of one file
enum { IRI_ROUTE = 0, IRI_LINES, IRI_SKIPPED, IRI_CELLS, IRI_MEMBERS, IRI_TEXT, IRI_WINDOWS, IRI_FLAGS, IRI_WORDS };

// What one vs_links_from_info call holds: every buffer dies with it.
struct InfoRead {
    vs_ctx *ctx = nullptr;
    uint32_t n = 0, window = 0;
    bool dense = true;
    int64_t *d_p0 = nullptr;
    IrNames names{};
    VsDevBuf d_blob, d_off, d_table, d_text[2], d_comp, d_dir, d_status, d_ctr, d_rows, d_cols, d_vals;
    std::vector<uint32_t> rows, cols;  // CSR route: the non-zero cells of both files
    std::vector<int64_t> vals;
    unsigned cur = 0;
    uint32_t text_cap = 0;

    int upload_names(const uint8_t *blob, const std::vector<uint64_t> &off0, const std::vector<IrSlot> &table, uint32_t bits) {
        const hipStream_t st = ctx->stream;
        const size_t blob_bytes = (size_t)off0.back();
        VS_HIP(ctx, d_blob.reserve(blob_bytes ? blob_bytes : 1u));
        VS_HIP(ctx, d_off.reserve(off0.size() * sizeof(uint64_t)));
        VS_HIP(ctx, d_table.reserve(table.size() * sizeof(IrSlot)));
        VS_HIP(ctx, d_ctr.reserve(IRC_WORDS * sizeof(uint32_t)));
        if (blob_bytes) VS_HIP(ctx, hipMemcpyAsync(d_blob.ptr(), blob, blob_bytes, hipMemcpyHostToDevice, st));
        VS_HIP(ctx, hipMemcpyAsync(d_off.ptr(), off0.data(), off0.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VS_HIP(ctx, hipMemcpyAsync(d_table.ptr(), table.data(), table.size() * sizeof(IrSlot), hipMemcpyHostToDevice, st));
        VS_HIP(ctx, hipStreamSynchronize(st));  // (the host arrays are the caller's and this function's locals)
        names.blob = d_blob.as<const uint8_t>(), names.off = d_off.as<const uint64_t>(), names.table = d_table.as<const IrSlot>();
        names.blob_bytes = blob_bytes, names.n = n, names.bits = bits;
        return VS_OK;
    }

    // both text buffers for a file of text_bytes bytes of text: a window at the most, a multiple of 16
    int reserve_text(uint64_t text_bytes) {
        const uint64_t want = (std::min<uint64_t>(std::max<uint64_t>(text_bytes, 1u), window) + 15u) / 16u * 16u;
        VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (VsDevBuf &b : d_text) VS_HIP(ctx, b.reserve((size_t)want));
        text_cap = (uint32_t)std::min<uint64_t>(d_text[0].capacity(), d_text[1].capacity()) / 16u * 16u;
        return VS_OK;
    }

    // The buffer d_text[cur] holds [0, size): w.carry bytes carried, then new text.  Scan, parse what the walk allows, carry
    // the tail into the other buffer and make that one current.  *bad: a malformed line was met (in this window or before).
    int window_step(IrWalk &w, uint32_t size, bool last, uint64_t st_out[IRI_WORDS], bool *bad) {
        const hipStream_t st = ctx->stream;
        uint32_t *ctr = d_ctr.as<uint32_t>();
        uint32_t h[IRC_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint8_t *txt = d_text[cur].as<const uint8_t>();
        st_out[IRI_WINDOWS]++;
        if (size) {
            VS_HIP(ctx, hipMemsetAsync(ctr, 0, IRC_WORDS * sizeof(uint32_t), st));
            const uint32_t chunks = (size + 15u) / 16u;
            const unsigned grid = (unsigned)std::min<uint32_t>((chunks + IR_TPB - 1u) / IR_TPB, 2048u);
            hipLaunchKernelGGL(k_info_scan, dim3(grid), dim3(IR_TPB), 0, st, txt, size, ctr);
            VS_HIP(ctx, hipGetLastError());
            VS_HIP(ctx, hipMemcpyAsync(h, ctr, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
        }
        const IrScan scan = {h[IRC_FLAGS], h[IRC_NEWLINES], h[IRC_EMPTY_INV] ? ~h[IRC_EMPTY_INV] : IR_NONE, h[IRC_NL_END]};
        if (scan.nl_end > size || (scan.empty != IR_NONE && scan.empty >= size)) return vs_fail(ctx, VS_E_STATE, "vs_links_from_info: the scan of a window of %u bytes answered %u / %u", size, scan.nl_end, scan.empty);
        st_out[IRI_FLAGS] |= scan.flags;
        const uint32_t limit = ir_walk_limit(w, scan, size, last);
        bool malformed = false;
        if (limit) {
            const uint32_t list_cap = dense ? 0u : scan.newlines + 1u;
            if (!dense) {
                VS_HIP(ctx, d_rows.reserve((size_t)list_cap * sizeof(uint32_t)));
                VS_HIP(ctx, d_cols.reserve((size_t)list_cap * sizeof(uint32_t)));
                VS_HIP(ctx, d_vals.reserve((size_t)list_cap * sizeof(int64_t)));
            }
            const uint32_t tiles = (limit + IR_TILE - 1u) / IR_TILE;
            const unsigned grid = (unsigned)std::min<uint32_t>(tiles, 2048u);
            if (dense)
                hipLaunchKernelGGL(k_info_parse<true>, dim3(grid), dim3(IR_TPB), 0, st, txt, size, text_cap, limit, names, n, d_p0, (uint32_t *)nullptr,
                                   (uint32_t *)nullptr, (int64_t *)nullptr, 0u, ctr);
            else
                hipLaunchKernelGGL(k_info_parse<false>, dim3(grid), dim3(IR_TPB), 0, st, txt, size, text_cap, limit, names, n, (int64_t *)nullptr,
                                   d_rows.as<uint32_t>(), d_cols.as<uint32_t>(), d_vals.as<int64_t>(), list_cap, ctr);
            VS_HIP(ctx, hipGetLastError());
            VS_HIP(ctx, hipMemcpyAsync(h + 4, ctr + 4, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
            malformed = h[IRC_BAD_INV] != 0u;
            if (!malformed) {
                st_out[IRI_LINES] += h[IRC_LINES], st_out[IRI_SKIPPED] += h[IRC_SKIPPED];
                if (h[IRC_CELLS] > list_cap) return vs_fail(ctx, VS_E_STATE, "vs_links_from_info: %u cells in a window of %u lines", h[IRC_CELLS], list_cap);
                if (const size_t m = h[IRC_CELLS]) {
                    const size_t at = rows.size();
                    rows.resize(at + m), cols.resize(at + m), vals.resize(at + m);
                    VS_HIP(ctx, hipMemcpyAsync(rows.data() + at, d_rows.ptr(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    VS_HIP(ctx, hipMemcpyAsync(cols.data() + at, d_cols.ptr(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    VS_HIP(ctx, hipMemcpyAsync(vals.data() + at, d_vals.ptr(), m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
                    VS_HIP(ctx, hipStreamSynchronize(st));
                }
            }
        }
        if (malformed) *bad = true;
        ir_walk_next(w, scan, size, malformed);
        if (w.carry) VS_HIP(ctx, hipMemcpyAsync(d_text[cur ^ 1u].ptr(), txt + (size - w.carry), w.carry, hipMemcpyDeviceToDevice, st));
        cur ^= 1u;
        return VS_OK;
    }

    // plain text, uploaded window by window from the mapped file
    int read_plain(const uint8_t *map, uint64_t size, uint64_t st_out[IRI_WORDS], int *outcome) {
        const hipStream_t st = ctx->stream;
        if (int rc = reserve_text(size)) return rc;
        IrWalk w = ir_walk_begin(window);
        bool bad = false;
        for (uint64_t at = 0; at < size;) {
            const uint32_t room = ir_walk_room(w);
            if (!room) return *outcome = IRO_HOST, VS_OK;  // a line longer than a window
            const uint32_t fresh = (uint32_t)std::min<uint64_t>(room, size - at), total = w.carry + fresh;
            if (total > text_cap) return vs_fail(ctx, VS_E_STATE, "vs_links_from_info: a window of %u bytes, room for %u", total, text_cap);
            VS_HIP(ctx, hipMemcpyAsync(d_text[cur].as<uint8_t>() + w.carry, map + at, fresh, hipMemcpyHostToDevice, st));
            at += fresh;
            st_out[IRI_TEXT] += fresh;
            if (int rc = window_step(w, total, at == size, st_out, &bad)) return rc;
        }
        *outcome = st_out[IRI_FLAGS] ? IRO_PYTHON : bad ? IRO_HOST : IRO_OK;
        return VS_OK;
    }

    // whole BGZF: the members of a window uploaded with their directory and inflated behind the carry
    int read_bgzf(const uint8_t *map, uint64_t size, const std::vector<uint64_t> &offsets, uint64_t st_out[IRI_WORDS], int *outcome) {
        const hipStream_t st = ctx->stream;
        const size_t nm = offsets.size() - 1u;
        std::vector<vs_bgzf_member> all(nm);
        uint64_t text_bytes = 0;
        for (size_t m = 0; m < nm; m++) {
            size_t msize = 0;
            if (offsets[m + 1] > size || offsets[m + 1] <= offsets[m] ||
                vs_bgzf_parse(map + offsets[m], (size_t)(offsets[m + 1] - offsets[m]), &all[m], &msize) != 0 || msize != offsets[m + 1] - offsets[m])
                return *outcome = IRO_HOST, VS_OK;  // (the walk said otherwise: the host reader words it)
            text_bytes += all[m].isize;
        }
        if (int rc = reserve_text(text_bytes)) return rc;
        IrWalk w = ir_walk_begin(window);
        bool bad = false;
        std::vector<vs_bgzf_member> dir;
        std::vector<uint32_t> status;
        for (size_t m0 = 0; m0 < nm;) {
            const uint32_t room = ir_walk_room(w);
            uint32_t fresh = 0;
            size_t m1 = m0;
            dir.clear();
            while (m1 < nm && all[m1].isize <= room - fresh) {
                vs_bgzf_member e = all[m1];
                if (offsets[m1] - offsets[m0] + e.in_off > 0xFFFF0000ull) break;
                e.in_off += (uint32_t)(offsets[m1] - offsets[m0]);
                e.out_off = w.carry + fresh;
                fresh += e.isize;
                dir.push_back(e);
                m1++;
            }
            if (m1 == m0) return *outcome = IRO_HOST, VS_OK;  // no member fits behind the line carried: it is longer than a window
            const uint32_t total = w.carry + fresh, k = (uint32_t)(m1 - m0);
            const size_t comp_bytes = (size_t)(offsets[m1] - offsets[m0]);
            if (total > text_cap) return vs_fail(ctx, VS_E_STATE, "vs_links_from_info: a window of %u bytes, room for %u", total, text_cap);
            if (d_comp.capacity() < comp_bytes || d_dir.capacity() < k * sizeof(vs_bgzf_member)) VS_HIP(ctx, hipStreamSynchronize(st));
            VS_HIP(ctx, d_comp.reserve(comp_bytes));
            VS_HIP(ctx, d_dir.reserve(k * sizeof(vs_bgzf_member)));
            VS_HIP(ctx, d_status.reserve(k * sizeof(uint32_t)));
            VS_HIP(ctx, hipMemcpyAsync(d_comp.ptr(), map + offsets[m0], comp_bytes, hipMemcpyHostToDevice, st));
            VS_HIP(ctx, hipMemcpyAsync(d_dir.ptr(), dir.data(), k * sizeof(vs_bgzf_member), hipMemcpyHostToDevice, st));
            VS_HIP(ctx, hipMemsetAsync(d_status.ptr(), 0xFF, k * sizeof(uint32_t), st));
            vs_launch_inflate(st, d_comp.as<const uint8_t>(), comp_bytes, d_text[cur].as<uint8_t>(), total, d_dir.as<const vs_bgzf_member>(), k,
                              d_status.as<uint32_t>(), nullptr, 0, 0);
            VS_HIP(ctx, hipGetLastError());
            status.resize(k);
            VS_HIP(ctx, hipMemcpyAsync(status.data(), d_status.ptr(), k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
            for (uint32_t i = 0; i < k; i++)
                if (status[i] != INF_OK) return *outcome = IRO_HOST, VS_OK;  // a corrupt member: the host reader words the error
            st_out[IRI_MEMBERS] += k;
            st_out[IRI_TEXT] += fresh;
            m0 = m1;
            if (int rc = window_step(w, total, m0 == nm, st_out, &bad)) return rc;
        }
        *outcome = st_out[IRI_FLAGS] ? IRO_PYTHON : bad ? IRO_HOST : IRO_OK;
        return VS_OK;
    }

    // the file through vs_info_parse on the host threads; its cells into the table (dense) or behind the cell list (CSR)
    int read_host(const char *path, const uint8_t *nblob, const uint64_t *name_off, uint64_t st_out[IRI_WORDS], int *outcome) {
        uint64_t inf[4] = {0, 0, 0, 0};
        const auto parse = [&](uint32_t *r, uint32_t *c, int64_t *v, uint64_t cap) -> int {
            const int rc = vs_info_parse(path, nblob, name_off, n, r, c, v, cap, inf);
            if (rc != VS_OK) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
            return VS_OK;
        };
        if (int rc = parse(nullptr, nullptr, nullptr, 0)) return rc;
        st_out[IRI_FLAGS] = inf[1];
        if (inf[1]) return *outcome = IRO_PYTHON, VS_OK;
        const uint64_t cap = inf[0];
        std::vector<uint32_t> r((size_t)cap + 1u), c((size_t)cap + 1u);
        std::vector<int64_t> v((size_t)cap + 1u);
        if (cap)
            if (int rc = parse(r.data(), c.data(), v.data(), cap)) return rc;
        if (inf[1]) return *outcome = IRO_PYTHON, VS_OK;
        const uint64_t cells = cap ? inf[0] : 0u;
        st_out[IRI_LINES] = inf[2], st_out[IRI_SKIPPED] = inf[3];
        if (dense) {
            if (int rc = vs_links_scatter_cells(ctx, d_p0, n, r.data(), c.data(), v.data(), cells)) return rc;
        } else {
            rows.insert(rows.end(), r.begin(), r.begin() + cells);
            cols.insert(cols.end(), c.begin(), c.begin() + cells);
            vals.insert(vals.end(), v.begin(), v.begin() + cells);
        }
        *outcome = IRO_OK;
        return VS_OK;
    }

    // one file by the route it can take (force_host: an earlier attempt handed it to the host reader)
    int read_file(const char *path, bool force_host, const uint8_t *nblob, const uint64_t *name_off, uint64_t st_out[IRI_WORDS], int *outcome) {
        for (int i = 0; i < IRI_WORDS; i++) st_out[i] = 0;
        Fd file;
        file.fd = open(path, O_RDONLY);
        if (file.fd < 0) return vs_fail(ctx, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
        struct stat sb;
        if (fstat(file.fd, &sb) != 0) return vs_fail(ctx, VS_E_ARG, "cannot stat %s: %s", path, strerror(errno));
        const uint64_t size = (uint64_t)sb.st_size;
        Map map;
        if (size && !force_host) {
            map.p = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, file.fd, 0);
            if (map.p == MAP_FAILED) return vs_fail(ctx, VS_E_OOM, "cannot map %s: %s", path, strerror(errno));
            map.n = (size_t)size;
        }
        const uint8_t *p = (const uint8_t *)map.p;
        int route = IR_ROUTE_PLAIN;
        std::vector<uint64_t> offsets;
        if (force_host) {
            route = IR_ROUTE_HOST;
        } else if (size >= 2u && p[0] == 0x1fu && p[1] == 0x8bu) {  // gzip: on the device when it is BGZF from the first byte to the last
            uint64_t walk[4] = {0, 0, 0, 0};
            if (int rc = vs_bgzf_walk_file(path, nullptr, 0, walk)) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
            route = IR_ROUTE_HOST;
            if (walk[2] == 0 && walk[1] == size && walk[3] == size && walk[0]) {
                offsets.assign((size_t)walk[0] + 1u, 0);
                if (int rc = vs_bgzf_walk_file(path, offsets.data(), offsets.size(), walk)) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
                if (walk[2] == 0 && walk[1] == size && walk[0] + 1u == offsets.size()) route = IR_ROUTE_BGZF;
            }
        }
        st_out[IRI_ROUTE] = (uint64_t)route;
        const uint64_t before = rows.size();
        int rc = VS_OK;
        if (route == IR_ROUTE_HOST) rc = read_host(path, nblob, name_off, st_out, outcome);
        else if (route == IR_ROUTE_BGZF) rc = read_bgzf(p, size, offsets, st_out, outcome);
        else if (size) rc = read_plain(p, size, st_out, outcome);
        else *outcome = IRO_OK;
        if (rc != VS_OK) return rc;
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return vs_fail(ctx, VS_E_HIP, "vs_links_from_info: the device failed while %s was read", path);
        st_out[IRI_CELLS] = st_out[IRI_LINES] - st_out[IRI_SKIPPED];
        if (*outcome != IRO_OK) rows.resize((size_t)before), cols.resize((size_t)before), vals.resize((size_t)before);
        return VS_OK;
    }
};

}  // namespace

extern "C" int vs_links_from_info(vs_ctx *ctx, const char *pe_path, const char *st_path, const uint8_t *names, const uint64_t *name_off, uint32_t n,
                                  uint32_t sparse_min_nodes, uint64_t window_bytes, vs_links **out, uint64_t info[16]) {
    if (!ctx || !pe_path || !st_path || !name_off || !out || !info || (n && !names)) return vs_fail(ctx, VS_E_ARG, "vs_links_from_info: bad argument");
    *out = nullptr;
    for (int i = 0; i < 16; i++) info[i] = 0;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> off0;
    std::vector<IrSlot> table;
    uint32_t bits = 1;
    if (!build_names(name_off, n, names, off0, table, &bits)) return vs_fail(ctx, VS_E_ARG, "vs_links_from_info: the name offsets must not decrease");
    const uint32_t min_nodes = sparse_min_nodes ? sparse_min_nodes : VS_LINKS_SPARSE_MIN;
    const char *paths[2] = {pe_path, st_path};
    bool force_host[2] = {false, false};
    for (int attempt = 0; attempt < 3; attempt++) {
        InfoRead R;
        R.ctx = ctx, R.n = n, R.window = clamp_window(window_bytes), R.dense = n < min_nodes;
        if (int rc = R.upload_names(names ? names + name_off[0] : nullptr, off0, table, bits)) return rc;
        vs_links *L = nullptr;
        if (R.dense)
            if (int rc = vs_links_dense_zeroed(ctx, "vs_links_from_info", n, &L, &R.d_p0)) return rc;
        int rc = VS_OK, outcome = IRO_OK;
        bool again = false;
        for (int f = 0; f < 2 && rc == VS_OK && outcome == IRO_OK; f++) {
            rc = R.read_file(paths[f], force_host[f], names, name_off, info + 8 * f, &outcome);
            if (rc == VS_OK && outcome == IRO_HOST) {
                // what the table holds of this file by now cannot be taken back: start over, this file through the host reader
                if (force_host[f]) rc = vs_fail(ctx, VS_E_STATE, "vs_links_from_info: %s was handed to the host reader twice", paths[f]);
                force_host[f] = again = true;
            }
        }
        (void)hipStreamSynchronize(ctx->stream);  // (R's buffers die here)
        if (rc != VS_OK || outcome != IRO_OK) {
            vs_links_abandon(ctx, L);
            if (rc != VS_OK) return rc;
            if (outcome == IRO_PYTHON) return VS_OK;  // *out stays NULL: the caller's own loop reads the files
            if (again) continue;
        }
        if (R.dense) {
            *out = L;
            return VS_OK;
        }
        if (ctx->links_spare.ptr()) {  // (a dense buffer set aside earlier is not needed: give it back)
            ctx->links_spare.reset();
            ctx->links_spare_n = 0;
        }
        return vs_links_csr_from_cells(ctx, R.rows.data(), R.cols.data(), R.vals.data(), R.rows.size(), n, out);
    }
    return vs_fail(ctx, VS_E_STATE, "vs_links_from_info: no route read the files");
}

// The host twin: text[0, size) through the same header and the same walk, one thread, host arrays.  The cells (zero counts
// included, as vs_info_parse gives them) go to rows / cols / vals in text order.
// info: [0] outcome -- 0 read, 1 Python's to read, 2 a malformed line, 3 a line that does not fit a window (the host reader's)
//       [1] lines  [2] lines skipped  [3] cells  [4] text offset of the first malformed line  [5] windows  [6] flags  [7] text bytes
extern "C" int vs_info_read_host(const uint8_t *text, uint64_t size, const uint8_t *names, const uint64_t *name_off, uint32_t n, uint64_t window_bytes,
                                 uint32_t *rows, uint32_t *cols, int64_t *vals, uint64_t cap, uint64_t info[8]) {
    if ((!text && size) || !name_off || !info || (n && !names) || (cap && (!rows || !cols || !vals)))
        return vs_fail(nullptr, VS_E_ARG, "vs_info_read_host: bad argument");
    for (int i = 0; i < 8; i++) info[i] = 0;
    std::vector<uint64_t> off0;
    std::vector<IrSlot> table;
    uint32_t bits = 1;
    if (!build_names(name_off, n, names, off0, table, &bits)) return vs_fail(nullptr, VS_E_ARG, "vs_info_read_host: the name offsets must not decrease");
    const IrNames nm = {names ? names + name_off[0] : nullptr, off0.data(), table.data(), off0[n], n, bits};
    const uint32_t window = clamp_window(window_bytes);
    std::vector<uint8_t> buf((size_t)std::min<uint64_t>(window, std::max<uint64_t>(size, 1u)));
    IrWalk w = ir_walk_begin(window);
    uint64_t cells = 0, bad_at = UINT64_MAX;
    uint32_t have = 0;  // bytes of buf in use: the carry
    for (uint64_t at = 0; at < size;) {
        const uint32_t room = ir_walk_room(w);
        if (!room) {
            info[0] = 3;
            return VS_OK;
        }
        const uint32_t fresh = (uint32_t)std::min<uint64_t>(room, size - at), total = w.carry + fresh;
        memcpy(buf.data() + have, text + at, fresh);
        at += fresh;
        const bool last = at == size;
        info[5]++;
        const IrScan scan = ir_scan_host(buf.data(), total);
        info[6] |= scan.flags;
        const uint32_t limit = ir_walk_limit(w, scan, total, last);
        const IrHostReader rd = {buf.data(), total};
        bool malformed = false;
        for (uint32_t p = 0; p < limit && !malformed;) {
            const uint32_t stop = ir_line_stop(rd, p, total);
            uint32_t r = 0, c = 0;
            int64_t v = 0;
            const int what = ir_parse_line(nm, rd, p, stop, &r, &c, &v);
            if (what == IR_MALFORMED) {
                malformed = true;
                bad_at = w.base + p;
                break;
            }
            info[1]++;
            if (what == IR_SKIPPED) info[2]++;
            else {
                if (cells >= cap) return vs_fail(nullptr, VS_E_RANGE, "vs_info_read_host: more than %llu cells", (unsigned long long)cap);
                rows[cells] = r, cols[cells] = c, vals[cells] = v;
                cells++;
            }
            p = stop + 1u;
        }
        ir_walk_next(w, scan, total, malformed);
        if (w.carry) memmove(buf.data(), buf.data() + (total - w.carry), w.carry);
        have = w.carry;
    }
    info[3] = cells, info[7] = size;
    if (info[6]) info[0] = 1;
    else if (bad_at != UINT64_MAX) info[0] = 2, info[4] = bad_at;
    return VS_OK;
}
