// Read blocks: ASCII -> 2-bit packing on the device, unpacking (test aid) and the on-device
// synthetic pair generator used by bench.py.
//
// Layout (see vs_internal.h): ends interleaved (2r = forward, 2r+1 = reverse), every end starts
// on a uint32 word, 16 bases per word, LSB first; meta[e] = length | flags << 24.
#include <algorithm>
#include <utility>
#include <vector>

#include "vs_internal.h"
#include "vs_bam_core.h"
#include "vs_pack_host.h"

#define TPB 256

// Where the characters of a block's ends come from: open(e) = end e, with its length `len` and its character at(p), p < len.
// For the ends kernel of a block built on the device, length(e, bad) = that length alone -- or `bad` set where the source cannot
// give one (its list names a record outside the window): the pack kernel then never runs, so open() need not test again.
// `singles`: the source yields singles blocks, its odd ends are absent and neither method is asked for them.
struct PackBytes {  // an end that lies in memory as it reads
    const uint8_t *q;
    uint32_t len;
    __device__ uint8_t at(uint32_t p) const { return q[p]; }
};
// the sequence line of record r of a window, without its newline
__device__ __forceinline__ PackBytes pack_line(const SlWin &w, uint32_t r) {
    const uint32_t start = w.ends[4u * r] + 1u;
    return PackBytes{w.txt + start, w.ends[4u * r + 1u] - start};
}
struct PackText {  // the caller's text: end e is ascii[aoff[e], aoff[e + 1])
    const uint8_t *ascii;
    const uint64_t *aoff;
    __device__ PackBytes open(uint32_t e) const {
        const uint64_t a = aoff[e];
        return PackBytes{ascii + a, (uint32_t)(aoff[e + 1] - a)};
    }
};
struct PackLines {  // the windows of the streamed ingest: end e is line 4 (e / 2) + 1 of file e & 1
    static constexpr bool singles = false;
    SlWin f0, f1;
    __device__ PackBytes open(uint32_t e) const { return pack_line((e & 1u) ? f1 : f0, e >> 1); }
    __device__ uint32_t length(uint32_t e, bool &) const { return open(e).len; }
};
struct PackRecords {  // ONE window of the interleaved ingest: end e is line 4 rec[e] + 1 of it
    static constexpr bool singles = false;
    SlWin w;
    const uint32_t *rec;
    __device__ PackBytes open(uint32_t e) const { return pack_line(w, rec[e]); }
    __device__ uint32_t length(uint32_t e, bool &) const { return open(e).len; }
};
struct PackSingles {  // ONE window, unpaired reads: even end e is line 4 r + 1 of it, r = rec[e / 2] (rec == NULL: first + e / 2)
    static constexpr bool singles = true;
    SlWin w;
    const uint32_t *rec;
    uint32_t first;
    __device__ PackBytes open(uint32_t e) const { return pack_line(w, rec ? rec[e >> 1] : first + (e >> 1)); }
    __device__ uint32_t length(uint32_t e, bool &) const { return open(e).len; }
};
struct PackPairs {  // TWO windows joined by name (vs_pair_names.hip): end e is line 4 rec[e] + 1 of file e & 1, n_rec[e & 1] records
    static constexpr bool singles = false;
    SlWin f0, f1;
    uint32_t n_rec[2];
    const uint32_t *rec;
    __device__ PackBytes open(uint32_t e) const { return pack_line((e & 1u) ? f1 : f0, rec[e]); }
    __device__ uint32_t length(uint32_t e, bool &bad) const {  // (every rec index range-tested: the join is new each round)
        const SlWin &w = (e & 1u) ? f1 : f0;
        const uint32_t r = rec[e];
        if (r < n_rec[e & 1u] && 4ull * r + 1u < w.n_nl) {
            const uint32_t start = w.ends[4u * r] + 1u, stop = w.ends[4u * r + 1u];
            if (start <= stop && stop <= w.size) return stop - start;
        }
        bad = true;
        return 0u;
    }
};
struct PackBamEnd {  // 4-bit bases, read backwards and complemented where the record's flag has 0x10
    const uint8_t *seq;
    uint32_t len;
    bool rev;
    __device__ uint8_t at(uint32_t p) const { return bam_base(seq, len, rev, p); }
};
// record r of the scanned window of the BAM ingest; its l_seq, or `bad` where the window has no record r
__device__ __forceinline__ PackBamEnd pack_bam_rec(const uint8_t *win, const uint32_t *recs, uint32_t r) {
    const uint32_t *q = recs + 4u * (size_t)r;
    return PackBamEnd{win + q[3], q[2], (q[1] & 0x10u) != 0u};
}
__device__ __forceinline__ uint32_t pack_bam_len(const uint32_t *recs, uint32_t n_rec, uint32_t r, bool &bad) {
    if (r < n_rec) return recs[4u * (size_t)r + 2u];
    bad = true;  // (never: the lists hold records of this window)
    return 0u;
}
struct PackBam {  // the records of a window of the BAM ingest: end e is record ends[e]
    static constexpr bool singles = false;
    BamEnds b;
    __device__ PackBamEnd open(uint32_t e) const { return pack_bam_rec(b.win, b.recs, b.ends[e]); }
    __device__ uint32_t length(uint32_t e, bool &bad) const { return pack_bam_len(b.recs, b.n_rec, b.ends[e], bad); }
};
struct PackBamSingles {  // the kept singletons of the BAM ingest: even end e is record list[e / 2] of the window
    static constexpr bool singles = true;
    BamSingles b;
    __device__ PackBamEnd open(uint32_t e) const { return pack_bam_rec(b.win, b.recs, b.list[e >> 1]); }
    __device__ uint32_t length(uint32_t e, bool &bad) const { return pack_bam_len(b.recs, b.n_rec, b.list[e >> 1], bad); }
};

// one thread per packed word; mask (may be NULL) beside the words
template <class Src>
__global__ void __launch_bounds__(TPB)
k_pack_reads(Src src, const uint32_t *__restrict__ woff, uint32_t n_ends, uint32_t total_words,
             uint32_t *__restrict__ words, uint32_t *__restrict__ mask, uint32_t *__restrict__ meta) {
    const uint32_t wi = blockIdx.x * TPB + threadIdx.x;
    if (wi >= total_words) return;
    const uint32_t e = vs_upper_idx(woff, n_ends + 1u, wi);
    const auto end = src.open(e);
    const uint32_t len = end.len;
    const uint32_t b0 = (wi - woff[e]) * 16u;
    uint32_t v = 0, m = 0, fl = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t p = b0 + i;
        if (p < len) {
            const uint8_t c = end.at(p);
            const uint32_t code = vs_code(c);
            if (code > 3u) {
                fl |= (c == 'N') ? VS_FLAG_N : VS_FLAG_INVALID;
                m |= 3u << (2 * i);
            }
            v |= (code & 3u) << (2 * i);
        }
    }
    words[wi] = v;
    if (mask) mask[wi] = m;
    if (fl) atomicOr(&meta[e], fl << 24);
}

// r's woff and meta (lengths) are on the device: its words, and the mask beside them, from the bytes at src
template <class Src>
static void launch_pack(hipStream_t st, const Src &src, const vs_reads *r) {
    if (r->n_words)
        hipLaunchKernelGGL(k_pack_reads<Src>, dim3((unsigned)((r->n_words + TPB - 1) / TPB)), dim3(TPB), 0, st, src, (const uint32_t *)r->d_woff,
                           (uint32_t)r->n_ends, (uint32_t)r->n_words, (uint32_t *)r->d_words, (uint32_t *)r->d_mask, (uint32_t *)r->d_meta);
}

// The lengths of a block built on the device: one thread per end (and one more for the closing word offset).  meta = the
// length of end e as its source gives it, wcnt = its packed words; the odd ends of a singles source are absent: no length, no
// words, VS_FLAG_ABSENT.  st: the builder's status words -- the longest end (atomicMax), the first end that stops the block
// (atomicMin; an end its source faults comes before any that is merely over the 24-bit limit: VS_BLK_OVER, e < 2^31).
template <class Src>
__global__ void __launch_bounds__(TPB)
k_block_ends(Src src, uint32_t n_ends, uint32_t *__restrict__ meta, uint32_t *__restrict__ wcnt, uint32_t *__restrict__ st) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e > n_ends) return;
    if (e == n_ends) {
        wcnt[e] = 0u;
        return;
    }
    if (Src::singles && (e & 1u)) {
        meta[e] = VS_FLAG_ABSENT << 24;
        wcnt[e] = 0u;
        return;
    }
    bool bad = false;
    const uint32_t len = src.length(e, bad);
    if (bad || len > VS_LEN_MASK) {
        atomicMin(&st[VS_BLK_BAD], bad ? e : e | VS_BLK_OVER);
        meta[e] = 0u;
        wcnt[e] = 0u;
        return;
    }
    meta[e] = len;
    wcnt[e] = (len + 15u) >> 4;
    atomicMax(&st[VS_BLK_MAXLEN], len);
}

__global__ void __launch_bounds__(TPB)
k_count_invalid(const uint32_t *__restrict__ meta, uint64_t n_ends, uint32_t *__restrict__ out) {
    uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    bool inv = e < n_ends && ((meta[e] >> 24) & VS_FLAG_INVALID);
    unsigned long long b = __ballot(inv);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(out, (uint32_t)__popcll(b));
}

// One thread per end: the positions of its bytes outside ACGT, read off the mask -- up to four of
// them, one byte each (0xFF = none), for vs_seed_limits in the straight-line mapping kernels; an end
// with more (or with one beyond position 254) is flagged VS_FLAG_MANY and takes the overflow path.
__global__ void __launch_bounds__(TPB)
k_inv4(const uint32_t *__restrict__ woff, const uint32_t *__restrict__ mask, uint64_t n_ends, uint32_t *__restrict__ meta,
       uint32_t *__restrict__ inv4) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= n_ends) return;
    const uint32_t m0 = meta[e];
    uint32_t out = 0xFFFFFFFFu;
    if ((m0 >> 24) & VS_FLAG_INVALID) {
        const uint32_t len = m0 & VS_LEN_MASK, nw = (len + 15u) >> 4;
        const uint32_t *mw = mask + woff[e];
        uint32_t count = 0;
        bool many = false;
        for (uint32_t wi = 0; wi < nw && !many; wi++) {
            uint32_t m = mw[wi];
            while (m) {
                const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                const uint32_t pos = wi * 16u + (bit >> 1);
                m &= ~(3u << (bit & ~1u));
                if (pos >= len) continue;
                if (count < 4u && pos < 255u) out = (out & ~(0xFFu << (8u * count))) | (pos << (8u * count));
                else many = true;
                count++;
            }
        }
        if (many) meta[e] = m0 | (VS_FLAG_MANY << 24);
    }
    inv4[e] = out;
}

__global__ void __launch_bounds__(TPB)
k_unpack_reads(VsReadsDev rd, const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= rd.n_ends) return;
    uint32_t len = rd.meta[e] & VS_LEN_MASK;
    const uint32_t *w = rd.words + rd.woff[e];
    uint8_t *o = out + out_off[e];
    for (uint32_t i = 0; i < len; i++) o[i] = "ACGT"[(w[i >> 4] >> ((i & 15u) * 2u)) & 3u];
}

// ---- a block's memory ----------------------------------------------------------------------------
// Grow-only cache of device buffers (vs_ctx::cache) that lends the blocks of the FASTQ ingests their arrays; NULL on
// allocation failure.
static void *cache_alloc(vs_ctx *ctx, size_t bytes) {
    if (!bytes) bytes = 16;
    for (auto &b : ctx->cache)
        if (!b.used && b.buf.capacity() >= bytes && b.buf.capacity() <= 2 * bytes + (1u << 20)) {
            b.used = true;
            return b.buf.ptr();
        }
    VsDevBuf buf;
    if (buf.reserve(bytes, bytes + bytes / 8) != hipSuccess) return nullptr;  // (blocks of one file differ a little in size)
    ctx->cache.push_back({std::move(buf), true});
    return ctx->cache.back().buf.ptr();
}

static void cache_release(vs_ctx *ctx, void *p) {
    if (!p) return;
    size_t idle = 0;
    for (auto &b : ctx->cache)
        if (b.buf.ptr() == p) b.used = false;
    for (auto &b : ctx->cache)
        if (!b.used) idle++;
    if (idle > 24) {  // do not hoard: drop the idle ones
        std::vector<vs_ctx::CachedBuf> keep;
        for (auto &b : ctx->cache)
            if (b.used) keep.push_back(std::move(b));
        ctx->cache.swap(keep);
    }
}

hipError_t vs_reads::alloc(vs_ctx *ctx, void *&view, size_t bytes) {
    if (cached) return (view = cache_alloc(ctx, bytes)) ? hipSuccess : hipErrorOutOfMemory;
    VsDevBuf *b = own;
    while (b->ptr()) b++;  // (five arrays, five slots)
    const hipError_t e = b->reserve(bytes);
    view = b->ptr();
    return e;
}

void vs_reads::release(vs_ctx *ctx, void *&view) {
    if (cached) cache_release(ctx, view);
    else
        for (VsDevBuf &b : own)
            if (view && b.ptr() == view) b.reset();
    view = nullptr;
}

hipError_t vs_reads_alloc(vs_ctx *ctx, hipStream_t st, vs_reads *r, uint64_t n_ends, const uint64_t *n_words, bool with_mask) {
    hipError_t e = hipSuccess;
    if (!r->d_woff) {
        const size_t b_woff = sizeof(uint32_t) * (n_ends + 1), b_meta = sizeof(uint32_t) * (n_ends ? n_ends : 1);
        r->n_ends = n_ends;
        if ((e = r->alloc(ctx, r->d_woff, b_woff)) != hipSuccess || (e = r->alloc(ctx, r->d_meta, b_meta)) != hipSuccess) return e;
        r->bytes = b_woff + b_meta;
    }
    if (!n_words) return e;
    const size_t b_words = sizeof(uint32_t) * (*n_words + VS_PAD_WORDS);
    r->n_words = *n_words;
    r->bytes += b_words;
    auto padded = [&](void *&a) {  // n_words words and the zero tail behind them
        const hipError_t e1 = r->alloc(ctx, a, b_words);
        return e1 != hipSuccess ? e1 : hipMemsetAsync((uint32_t *)a + r->n_words, 0, sizeof(uint32_t) * VS_PAD_WORDS, st);
    };
    if ((e = padded(r->d_words)) == hipSuccess && with_mask) e = padded(r->d_mask);
    return e;
}

hipError_t vs_reads_finish(vs_ctx *ctx, hipStream_t st, vs_reads *r, uint32_t *d_cnt, uint32_t *h_cnt) {
    const unsigned nbe = (unsigned)((r->n_ends + TPB - 1) / TPB);
    if (nbe) hipLaunchKernelGGL(k_count_invalid, dim3(nbe), dim3(TPB), 0, st, (const uint32_t *)r->d_meta, r->n_ends, d_cnt);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, sizeof *h_cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    r->n_invalid = *h_cnt;
    if (!r->n_invalid) {
        if (ctx->keep_masks && r->d_mask) r->bytes += sizeof(uint32_t) * (r->n_words + VS_PAD_WORDS);  // (vs_ctx_keep_masks: the 'N's stay visible)
        else r->release(ctx, r->d_mask);
        return hipSuccess;
    }
    // rare: some end holds a byte outside ACGTN -> the mask stays, and the position lists are read off it
    if ((e = r->alloc(ctx, r->d_inv4, sizeof(uint32_t) * r->n_ends)) != hipSuccess) return e;
    r->bytes += sizeof(uint32_t) * (r->n_words + VS_PAD_WORDS) + sizeof(uint32_t) * r->n_ends;
    hipLaunchKernelGGL(k_inv4, dim3(nbe), dim3(TPB), 0, st, (const uint32_t *)r->d_woff, (const uint32_t *)r->d_mask, r->n_ends,
                       (uint32_t *)r->d_meta, (uint32_t *)r->d_inv4);
    return hipGetLastError();
}

// THE builder of a block cut on the device (VsBlockJob, vs_internal.h): every streamed ingest ends here.
template <class Src>
static hipError_t build_block(const VsBlockJob &j, const Src &src, vs_reads **out) {
    *out = nullptr;
    vs_ctx *ctx = j.ctx;
    hipStream_t st = j.st;
    const uint64_t n_ends = j.n_ends;
    const size_t b_wcnt = sizeof(uint32_t) * (n_ends + 1u);
    hipError_t e = j.wcnt->reserve(b_wcnt, b_wcnt + b_wcnt / 4u);  // (the stream is idle between blocks: nothing still reads it)
    if (e != hipSuccess) return e;
    uint32_t *wcnt = j.wcnt->as<uint32_t>();
    vs_reads *r = new vs_reads();
    r->cached = true;
    r->unpaired = Src::singles;
    auto fail = [&](hipError_t e1) {  // (the block goes back)
        vs_reads_free(ctx, r);
        return e1;
    };
    if ((e = vs_reads_alloc(ctx, st, r, n_ends, nullptr, true)) != hipSuccess) return fail(e);
    e = hipMemsetAsync(j.d_st, 0, sizeof(uint32_t) * VS_BLK_ST, st);
    if (e == hipSuccess) e = hipMemsetAsync(j.d_st + VS_BLK_BAD, 0xFF, sizeof(uint32_t), st);
    if (e != hipSuccess) return fail(e);
    hipLaunchKernelGGL(k_block_ends<Src>, dim3((unsigned)((n_ends + 1u + TPB - 1u) / TPB)), dim3(TPB), 0, st, src, (uint32_t)n_ends, (uint32_t *)r->d_meta, wcnt,
                       j.d_st);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    vs_launch_scan_u32(st, wcnt, (uint32_t)(n_ends + 1u), j.d_st + VS_BLK_WORDS);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    e = hipMemcpyAsync(r->d_woff, wcnt, sizeof(uint32_t) * (n_ends + 1u), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(j.h_st, j.d_st, sizeof(uint32_t) * j.n_st, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    if (j.h_st[VS_BLK_BAD] != 0xFFFFFFFFu) return fail(hipSuccess);  // no block: the caller words what VS_BLK_BAD says
    const uint64_t words = j.h_st[VS_BLK_WORDS];
    r->max_len = j.h_st[VS_BLK_MAXLEN];
    if ((e = vs_reads_alloc(ctx, st, r, n_ends, &words, true)) != hipSuccess) return fail(e);
    launch_pack(st, src, r);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = vs_reads_finish(ctx, st, r, j.d_st + VS_BLK_INVALID, j.h_st + VS_BLK_INVALID)) != hipSuccess) return fail(e);
    if (!j.more && (e = hipStreamSynchronize(st)) != hipSuccess) return fail(e);  // (the block is complete when it is handed out)
    *out = r;
    return hipSuccess;
}
hipError_t vs_block_lines(const VsBlockJob &j, const SlWin &f0, const SlWin &f1, vs_reads **out) { return build_block(j, PackLines{f0, f1}, out); }
hipError_t vs_block_records(const VsBlockJob &j, const SlWin &w, const uint32_t *rec, vs_reads **out) { return build_block(j, PackRecords{w, rec}, out); }
hipError_t vs_block_singles(const VsBlockJob &j, const SlWin &w, const uint32_t *rec, uint32_t first, vs_reads **out) { return build_block(j, PackSingles{w, rec, first}, out); }
hipError_t vs_block_pairs(const VsBlockJob &j, const SlWin &f0, uint32_t n_rec0, const SlWin &f1, uint32_t n_rec1, const uint32_t *rec, vs_reads **out) {
    return build_block(j, PackPairs{f0, f1, {n_rec0, n_rec1}, rec}, out);
}
hipError_t vs_block_bam(const VsBlockJob &j, const BamEnds &b, vs_reads **out) { return build_block(j, PackBam{b}, out); }
hipError_t vs_block_bam_singles(const VsBlockJob &j, const BamSingles &b, vs_reads **out) { return build_block(j, PackBamSingles{b}, out); }

extern "C" void vs_reads_free(vs_ctx *ctx, vs_reads *r) {
    if (!r) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        for (void **a : {&r->d_woff, &r->d_meta, &r->d_words, &r->d_mask, &r->d_inv4}) r->release(ctx, *a);
    }
    delete r;  // (what the block still owns goes with it)
}

extern "C" int vs_reads_info(const vs_reads *r, uint64_t info[5]) {
    if (!r || !info) return VS_E_ARG;
    info[0] = r->n_ends; info[1] = r->n_words; info[2] = r->max_len; info[3] = r->n_invalid; info[4] = r->bytes;
    return VS_OK;
}

// the device side of vs_reads_pack: woff / meta are the host's word offsets and lengths
static int pack_block(vs_ctx *ctx, vs_reads *r, const uint8_t *ascii, const uint64_t *off, const std::vector<uint32_t> &woff, const std::vector<uint32_t> &meta) {
    const uint64_t n_ends = woff.size() - 1, words = woff[n_ends], total = off[n_ends];
    hipStream_t st = ctx->stream;
    VS_HIP(ctx, vs_reads_alloc(ctx, st, r, n_ends, &words, true));
    VsDevBuf ascii_buf, aoff_buf, cnt_buf;
    VS_HIP(ctx, ascii_buf.reserve(total + 16));
    VS_HIP(ctx, aoff_buf.reserve(sizeof(uint64_t) * (n_ends + 1)));
    VS_HIP(ctx, cnt_buf.reserve(sizeof(uint32_t)));
    if (total) VS_HIP(ctx, hipMemcpyAsync(ascii_buf.ptr(), ascii, total, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(aoff_buf.ptr(), off, sizeof(uint64_t) * (n_ends + 1), hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(r->d_woff, woff.data(), sizeof(uint32_t) * (n_ends + 1), hipMemcpyHostToDevice, st));
    if (n_ends) VS_HIP(ctx, hipMemcpyAsync(r->d_meta, meta.data(), sizeof(uint32_t) * n_ends, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(cnt_buf.ptr(), 0, sizeof(uint32_t), st));
    launch_pack(st, PackText{ascii_buf.as<uint8_t>(), aoff_buf.as<uint64_t>()}, r);
    uint32_t h_cnt = 0;
    VS_HIP(ctx, vs_reads_finish(ctx, st, r, cnt_buf.as<uint32_t>(), &h_cnt));
    VS_HIP(ctx, hipStreamSynchronize(st));  // (the temporaries die here)
    return VS_OK;
}

// vs_reads_pack / vs_reads_pack_single: the host's word offsets and lengths of n_ends ends of ascii/off, then the device side
static int pack_text(vs_ctx *ctx, const char *who, const uint8_t *ascii, const uint64_t *off, uint64_t n_ends, bool unpaired, vs_reads **out) {
    if (n_ends > 0xFFFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "%s: split the input into blocks of < 2^32 ends", who);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> woff(n_ends + 1), meta(n_ends ? n_ends : 1);
    uint64_t words = 0, maxlen = 0;
    for (uint64_t e = 0; e < n_ends; e++) {
        uint64_t len = off[e + 1] - off[e];
        if (len > VS_LEN_MASK) return vs_fail(ctx, VS_E_RANGE, "read end %llu is %llu bytes long", (unsigned long long)e, (unsigned long long)len);
        woff[e] = (uint32_t)words;
        meta[e] = (uint32_t)len | ((unpaired && (e & 1ull)) ? VS_FLAG_ABSENT << 24 : 0u);
        words += (len + 15) / 16;
        if (len > maxlen) maxlen = len;
        if (words > 0xFFFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "%s: block exceeds 2^32 packed words", who);
    }
    woff[n_ends] = (uint32_t)words;
    vs_reads *r = new vs_reads();
    r->max_len = maxlen;
    r->unpaired = unpaired;
    int rc = pack_block(ctx, r, ascii, off, woff, meta);
    if (rc != VS_OK) { vs_reads_free(ctx, r); return rc; }
    *out = r;
    return VS_OK;
}

extern "C" int vs_reads_pack(vs_ctx *ctx, const uint8_t *ascii, const uint64_t *off, uint64_t n_ends, vs_reads **out) {
    if (!ctx || !off || !out) return VS_E_ARG;
    *out = nullptr;
    if (n_ends & 1ull) return vs_fail(ctx, VS_E_ARG, "vs_reads_pack: ends come in pairs (got %llu)", (unsigned long long)n_ends);
    return pack_text(ctx, "vs_reads_pack", ascii, off, n_ends, false, out);
}

// A singles block: read r is end 2r, end 2r + 1 is the empty range behind it, flagged absent
extern "C" int vs_reads_pack_single(vs_ctx *ctx, const uint8_t *ascii, const uint64_t *off, uint64_t n_reads, vs_reads **out) {
    if (!ctx || !off || !out) return VS_E_ARG;
    *out = nullptr;
    if (n_reads > 0x7FFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "vs_reads_pack_single: split the input into blocks of < 2^31 reads");
    std::vector<uint64_t> off2(2 * n_reads + 1);
    for (uint64_t r = 0; r < n_reads; r++) {
        off2[2 * r] = off[r];
        off2[2 * r + 1] = off[r + 1];
    }
    off2[2 * n_reads] = off[n_reads];
    return pack_text(ctx, "vs_reads_pack_single", ascii, off2.data(), 2 * n_reads, true, out);
}

extern "C" int vs_reads_unpaired(const vs_reads *r) { return r && r->unpaired ? 1 : 0; }

extern "C" int vs_reads_unpack(vs_ctx *ctx, const vs_reads *r, uint8_t *out, uint32_t *lens, uint8_t *flags) {
    if (!ctx || !r || !out) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> meta(r->n_ends ? r->n_ends : 1);
    if (r->n_ends) VS_HIP(ctx, hipMemcpyAsync(meta.data(), r->d_meta, sizeof(uint32_t) * r->n_ends, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ooff(r->n_ends + 1);
    uint64_t tot = 0;
    for (uint64_t e = 0; e < r->n_ends; e++) {
        ooff[e] = tot;
        tot += meta[e] & VS_LEN_MASK;
        if (lens) lens[e] = meta[e] & VS_LEN_MASK;
        if (flags) flags[e] = (uint8_t)(meta[e] >> 24);
    }
    ooff[r->n_ends] = tot;
    if (!tot) return VS_OK;
    VsDevBuf ooff_buf, out_buf;
    VS_HIP(ctx, ooff_buf.reserve(sizeof(uint64_t) * (r->n_ends + 1)));
    VS_HIP(ctx, out_buf.reserve(tot));
    uint64_t *d_ooff = ooff_buf.as<uint64_t>();
    uint8_t *d_out = out_buf.as<uint8_t>();
    VS_HIP(ctx, hipMemcpyAsync(d_ooff, ooff.data(), sizeof(uint64_t) * (r->n_ends + 1), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_unpack_reads, dim3((unsigned)((r->n_ends + TPB - 1) / TPB)), dim3(TPB), 0, ctx->stream, r->dev(), d_ooff, d_out);
    VS_HIP(ctx, hipMemcpyAsync(out, d_out, tot, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VS_OK;
}

// ---- synthetic pairs ---------------------------------------------------------------------------
// Integer recipe shared with oracle/pe_oracle.c:peo_synth_pairs (the CPU twin).  One thread per
// output word.
struct SynthParams {
    const uint32_t *gwords;  // packed genomes
    const uint64_t *gbase;   // [n_strains] first base (multiple of 16) of each genome in gwords
    const uint64_t *glen;    // [n_strains]
    const uint32_t *cum;     // [n_strains]
    uint32_t n_strains;
    uint64_t seed, first_pair, n_pairs;
    uint32_t read_len, words_per_end, sub_thresh, n_thresh;
};

__device__ __forceinline__ uint32_t gbase_at(const uint32_t *w, uint64_t i) {
    return (w[i >> 4] >> ((uint32_t)(i & 15u) * 2u)) & 3u;
}

__global__ void __launch_bounds__(TPB)
k_synth(SynthParams P, uint32_t *__restrict__ words, uint32_t *__restrict__ meta) {
    uint64_t t = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    uint64_t per_pair = 2ull * P.words_per_end;
    if (t >= P.n_pairs * per_pair) return;
    uint64_t q = t / per_pair;
    uint32_t rem = (uint32_t)(t - q * per_pair);
    uint32_t e = rem / P.words_per_end, wi = rem - e * P.words_per_end;
    uint64_t r = P.first_pair + q;
    uint64_t base = vs_mix64(P.seed * 0xD1342543DE82EF95ull + r);
    uint64_t u0 = vs_mix64(base + 1), u1 = vs_mix64(base + 2), u2 = vs_mix64(base + 3), u3 = vs_mix64(base + 4);
    uint32_t pick = (uint32_t)(u0 >> 32), s = 0;
    while (s + 1 < P.n_strains && pick > P.cum[s]) s++;
    int64_t L = P.read_len, glen = (int64_t)P.glen[s];
    int64_t sum = (int64_t)(u1 & 0xFFFF) + (int64_t)((u1 >> 16) & 0xFFFF) + (int64_t)((u1 >> 32) & 0xFFFF) + (int64_t)((u1 >> 48) & 0xFFFF);
    int64_t flen = 3 * L + (sum - 131070) * (3 * L) / 378372;
    if (flen < L) flen = L;
    if (flen > glen) flen = glen;
    int64_t start = (int64_t)((u2 >> 11) % (uint64_t)(glen - flen + 1));
    uint32_t flip = (uint32_t)(u2 & 1ull);
    // end e reads forward from `start` when (e == flip), else reverse-complemented from the far end
    bool forward = (e == flip);
    uint64_t g0 = P.gbase[s];
    uint32_t n_thr_hit = ((uint32_t)u3 < P.n_thresh) ? 1u : 0u;
    uint32_t n_end = (uint32_t)(u3 >> 62) & 1u;
    uint32_t n_pos = (uint32_t)((u3 >> 32) & 0x3FFFFFFFu) % P.read_len;
    uint32_t v = 0;
    for (uint32_t i = 0; i < 16; i++) {
        int64_t p = (int64_t)wi * 16 + i;
        if (p >= L) break;
        uint32_t b = forward ? gbase_at(P.gwords, g0 + (uint64_t)(start + p))
                             : (gbase_at(P.gwords, g0 + (uint64_t)(start + flen - 1 - p)) ^ 3u);
        if (P.sub_thresh) {
            uint64_t h = vs_mix64(base + 16 + (uint64_t)e * 4096 + (uint64_t)p);
            if ((uint32_t)h < P.sub_thresh) b = (b + 1u + (uint32_t)((h >> 32) % 3ull)) & 3u;
        }
        v |= b << (2 * i);
    }
    uint64_t end_id = 2 * q + e;
    words[end_id * P.words_per_end + wi] = v;
    if (wi == 0) {
        uint32_t fl = (n_thr_hit && n_end == e) ? VS_FLAG_N : 0u;
        (void)n_pos;  // the N's position does not matter once the pair is flagged
        meta[end_id] = P.read_len | (fl << 24);
    }
}

__global__ void __launch_bounds__(TPB) k_iota_woff(uint32_t *woff, uint64_t n, uint32_t stride) {
    uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) woff[i] = (uint32_t)(i * stride);
}

// the device side of vs_synth_pairs
static int synth_block(vs_ctx *ctx, vs_reads *r, uint64_t n_ends, const std::vector<uint32_t> &gwords, const std::vector<uint64_t> &gbase, const std::vector<uint64_t> &glen,
                       const uint32_t *cum, uint64_t seed, uint64_t first_pair, uint32_t read_len, uint32_t sub_thresh, uint32_t n_thresh) {
    const uint32_t n_strains = (uint32_t)gbase.size(), wpe = (read_len + 15) / 16;
    hipStream_t st = ctx->stream;
    const uint64_t n_words = n_ends * wpe;
    VS_HIP(ctx, vs_reads_alloc(ctx, st, r, n_ends, &n_words, false));
    VsDevBuf d_gw, d_cum, d_gb, d_gl;
    VS_HIP(ctx, d_gw.reserve(sizeof(uint32_t) * gwords.size()));
    VS_HIP(ctx, d_cum.reserve(sizeof(uint32_t) * n_strains));
    VS_HIP(ctx, d_gb.reserve(sizeof(uint64_t) * n_strains));
    VS_HIP(ctx, d_gl.reserve(sizeof(uint64_t) * n_strains));
    VS_HIP(ctx, hipMemcpyAsync(d_gw.ptr(), gwords.data(), sizeof(uint32_t) * gwords.size(), hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(d_cum.ptr(), cum, sizeof(uint32_t) * n_strains, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(d_gb.ptr(), gbase.data(), sizeof(uint64_t) * n_strains, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemcpyAsync(d_gl.ptr(), glen.data(), sizeof(uint64_t) * n_strains, hipMemcpyHostToDevice, st));
    SynthParams P;
    P.gwords = d_gw.as<uint32_t>(); P.gbase = d_gb.as<uint64_t>(); P.glen = d_gl.as<uint64_t>(); P.cum = d_cum.as<uint32_t>(); P.n_strains = n_strains;
    P.seed = seed; P.first_pair = first_pair; P.n_pairs = r->n_ends / 2; P.read_len = read_len;
    P.words_per_end = wpe; P.sub_thresh = sub_thresh; P.n_thresh = n_thresh;
    uint64_t nthreads = r->n_words;
    if (nthreads)
        hipLaunchKernelGGL(k_synth, dim3((unsigned)((nthreads + TPB - 1) / TPB)), dim3(TPB), 0, st, P,
                           (uint32_t *)r->d_words, (uint32_t *)r->d_meta);
    hipLaunchKernelGGL(k_iota_woff, dim3((unsigned)((r->n_ends + 1 + TPB - 1) / TPB)), dim3(TPB), 0, st,
                       (uint32_t *)r->d_woff, r->n_ends + 1, wpe);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipStreamSynchronize(st));  // (the temporaries die here)
    return VS_OK;
}

extern "C" int vs_synth_pairs(vs_ctx *ctx, const uint8_t *genomes, const uint64_t *goff, const uint32_t *cum,
                              uint32_t n_strains, uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint32_t read_len,
                              uint32_t sub_thresh, uint32_t n_thresh, vs_reads **out) {
    if (!ctx || !genomes || !goff || !cum || !out || !n_strains) return VS_E_ARG;
    *out = nullptr;
    if (read_len == 0 || read_len > 4096) return vs_fail(ctx, VS_E_ARG, "vs_synth_pairs: read_len must be 1..4096");
    uint32_t wpe = (read_len + 15) / 16;
    if (2 * n_pairs * wpe > 0xFFFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "vs_synth_pairs: block exceeds 2^32 packed words");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    // pack the genomes on the host (tiny) into word-aligned 2-bit text
    std::vector<uint64_t> gbase(n_strains), glen(n_strains);
    uint64_t gw = 0;
    for (uint32_t s = 0; s < n_strains; s++) {
        gbase[s] = gw * 16;
        glen[s] = goff[s + 1] - goff[s];
        if (glen[s] < read_len) return vs_fail(ctx, VS_E_ARG, "vs_synth_pairs: genome %u shorter than a read", s);
        gw += (glen[s] + 15) / 16;
    }
    std::vector<uint32_t> gwords(gw + 4, 0u);
    for (uint32_t s = 0; s < n_strains; s++)
        for (uint64_t i = 0; i < glen[s]; i += 1u << 30)  // (the packer takes a 32-bit length)
            if (vs_pack_sequence_host_plain(genomes + goff[s] + i, (uint32_t)std::min<uint64_t>(glen[s] - i, 1u << 30), &gwords[(gbase[s] + i) >> 4]))
                return vs_fail(ctx, VS_E_ARG, "vs_synth_pairs: genome %u holds a byte outside ACGT", s);
    vs_reads *r = new vs_reads();
    r->max_len = read_len;
    int rc = synth_block(ctx, r, 2 * n_pairs, gwords, gbase, glen, cum, seed, first_pair, read_len, sub_thresh, n_thresh);
    if (rc != VS_OK) { vs_reads_free(ctx, r); return rc; }
    *out = r;
    return VS_OK;
}
