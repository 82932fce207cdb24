// The host reader of the streamed ingests (vs_stream.hip: two FASTQ files; vs_interleaved.hip: one interleaved FASTQ; vs_bam.hip: BAM): one file read front to back by a thread of
// its own into a bounded ring of pinned chunks -- plain bytes, zlib-inflated gzip, the raw deflate payloads of whole BGZF
// members with their directory, or (VS_GZIP_DEVICE=1) the bytes of a plain gzip file as they are, for the device to inflate
// (see the top of vs_stream.hip).
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "vs_internal.h"

namespace {

constexpr size_t STREAM_CHUNK_BYTES = 64u << 20;  // one pinned chunk of the ring; VS_STREAM_CHUNK overrides it (tests only)
constexpr unsigned STREAM_RING_SLOTS = 4;         // chunks per file in the ring
constexpr size_t STREAM_MAX_WINDOW = 0xFFFFFF00u; // line ends and record starts are 32-bit byte offsets into a window
enum { M_PLAIN = 0, M_ZLIB = 1, M_BGZF = 2, M_GZRAW = 3 };

struct Slot {
    VsPinnedBuf buf;          // slot_cap bytes, pinned by the reader at first use
    size_t len = 0;  // bytes of text, or of deflate payloads when n_members > 0 or comp
    bool last = false;
    bool comp = false;        // payloads of BGZF members + their directory at the slot's end (the last member first)
    bool gz = false;          // the next bytes of a plain gzip file, not inflated (text = 0: the device finds out)
    uint32_t n_members = 0;
    size_t text = 0;          // what the members inflate to (the ISIZE sum)
};
// member i of a BGZF slot (its directory grows down from the slot's end)
inline const vs_bgzf_member &slot_member(const Slot &sl, uint32_t i) {
    return ((const vs_bgzf_member *)(sl.buf.as<uint8_t>() + sl.buf.capacity()))[-(ptrdiff_t)(i + 1u)];
}

// n bytes of fd from offset off (EINTR retried): nullptr, or why not -- for "cannot read %s: %s"
inline const char *pread_all(int fd, void *dst, size_t n, uint64_t off) {
    for (size_t have = 0; have < n;) {
        const ssize_t got = pread(fd, (uint8_t *)dst + have, n - have, (off_t)(off + have));
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) return got < 0 ? strerror(errno) : "it shrank while it was read";
        have += (size_t)got;
    }
    return nullptr;
}

// One file read front to back by a thread of its own into the ring.  The consumer takes filled slots in order and gives
// them back once their bytes are on the device.
struct Reader {
    std::string path;
    int fd = -1, device = 0;
    size_t chunk = STREAM_CHUNK_BYTES;
    Slot slots[STREAM_RING_SLOTS];
    uint64_t filled = 0, taken = 0;  // slots published / given back (monotonic)
    bool stop = false, finished = false;
    int err = VS_OK;
    std::string err_msg;
    bool gzip = false, bgzf = false, bgzf_device = true, gzip_device = false, gz_raw = false;
    size_t slot_cap = STREAM_CHUNK_BYTES;
    uint64_t raw_bytes = 0, text_bytes = 0, members_host = 0;
    uint64_t begin = 0, end = ~0ull;  // the bytes of the file this reader may read (a member range of a sharded open)
    std::mutex m;
    std::condition_variable cv;
    std::thread th;

    // the file opened for a reader on the context's device (VS_STREAM_CHUNK: tests, records across chunks)
    int open_file(vs_ctx *ctx, const char *p) {
        path = p;
        device = ctx->device;
        if (const char *ev = getenv("VS_STREAM_CHUNK")) chunk = std::max<size_t>(1u, (size_t)atoll(ev));
        fd = open(p, O_RDONLY);
        return fd < 0 ? cannot_open(ctx, errno) : VS_OK;
    }
    int cannot_open(vs_ctx *ctx, int e) {
        if (fd >= 0) close(fd);
        fd = -1;
        return vs_fail(ctx, VS_E_ARG, "cannot open %s: %s", path.c_str(), strerror(e));
    }
    int fail(int code, const char *fmt, const char *a, const char *b = "") {
        char buf[512];
        snprintf(buf, sizeof buf, fmt, a, b);
        err = code;
        err_msg = buf;
        return code;
    }
    // read(2) up to n bytes; 0 at the end of the file; -1 on an error or when asked to stop
    ssize_t raw_read(uint8_t *dst, size_t n) {
        for (;;) {
            {
                std::lock_guard<std::mutex> lk(m);
                if (stop) return -1;
            }
            struct pollfd pfd = {fd, POLLIN, 0};
            const int pr = poll(&pfd, 1, 200);  // (a pipe whose writer is slow: look at `stop` now and then)
            if (pr == 0 || (pr < 0 && errno == EINTR)) continue;
            const uint64_t left = end - (begin + raw_bytes);  // (never a byte beyond the range, not even into a buffer)
            if (left == 0) return 0;
            const ssize_t got = read(fd, dst, (size_t)std::min<uint64_t>(std::min<size_t>(n, 1u << 30), left));
            if (got < 0 && errno == EINTR) continue;
            if (got < 0) {
                fail(VS_E_ARG, "cannot read %s: %s", path.c_str(), strerror(errno));
                return -1;
            }
            raw_bytes += (uint64_t)got;
            return got;
        }
    }
    void run() {
        (void)hipSetDevice(device);
        if (begin && lseek(fd, (off_t)begin, SEEK_SET) < 0) {
            fail(VS_E_ARG, "cannot seek in %s: %s", path.c_str(), strerror(errno));
            publish(0, true);
            return;
        }
        std::vector<uint8_t> in(1u << 20);
        size_t in_len = 0;
        bool in_eof = false;
        // the first bytes say whether the file is gzip (magic 1f 8b)
        while (in_len < 18 && !in_eof) {  // (18: the header of a BGZF member as bgzip writes it)
            const ssize_t got = raw_read(in.data() + in_len, in.size() - in_len);
            if (got < 0) { publish(0, true); return; }
            if (got == 0) in_eof = true;
            in_len += (size_t)got;
        }
        gzip = in_len >= 2 && in[0] == 0x1f && in[1] == 0x8b;
        int mode = gzip ? M_ZLIB : M_PLAIN;
        if (gzip && bgzf_device) {
            vs_bgzf_member mb;
            size_t msize = 0;
            if (vs_bgzf_parse(in.data(), in_len, &mb, &msize) != 2) mode = M_BGZF;
        }
        if (mode == M_ZLIB && gzip_device) mode = M_GZRAW;  // (a file whose first member is BGZF keeps the BGZF path)
        bgzf = mode == M_BGZF;
        gz_raw = mode == M_GZRAW;
        slot_cap = bgzf ? (std::max<size_t>(chunk, 65536u) + 15u) & ~(size_t)15u : chunk;
        size_t in_at = 0;  // (BGZF: bytes of `in` already handed on)
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        const bool zs_open = gzip && mode != M_GZRAW;  // (M_GZRAW makes no zlib call)
        if (zs_open && inflateInit2(&zs, 15 + 16) != Z_OK) {
            fail(VS_E_OOM, "%s: zlib cannot start", path.c_str());
            publish(0, true);
            return;
        }
        size_t plain_at = 0;  // (plain text: bytes of `in` not yet handed on)
        if (mode == M_ZLIB) {
            zs.next_in = in.data();
            zs.avail_in = (uInt)in_len;
        }
        bool at_end = false;
        while (!at_end) {
            Slot *slot = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || filled - taken < STREAM_RING_SLOTS; });
                if (stop) break;
                slot = &slots[filled % STREAM_RING_SLOTS];  // (free: the consumer gave it back)
            }
            if (slot->buf.reserve(slot_cap) != hipSuccess)
                fail(VS_E_OOM, "%s: cannot pin a %s-byte chunk", path.c_str(), std::to_string(slot_cap).c_str());
            uint8_t *dst = slot->buf.as<uint8_t>();
            if (!dst) { publish(0, true); break; }
            size_t len = 0;
            bool bad = false;
            if (mode == M_BGZF) {
                uint32_t nm = 0;
                size_t text = 0;
                bool to_zlib = false;
                vs_bgzf_member *dir_end = (vs_bgzf_member *)(dst + slot_cap);
                for (;;) {
                    vs_bgzf_member mb;
                    size_t msize = 0;
                    const int st = vs_bgzf_parse(in.data() + in_at, in_len - in_at, &mb, &msize);
                    if (st == 0) {
                        const size_t need = ((len + mb.in_len + 3u) & ~(size_t)3u) + sizeof(vs_bgzf_member) * (nm + 1u);
                        if (nm && (need > slot_cap || text + mb.isize > chunk || len + mb.in_len > 0xFFFF0000u)) break;  // the next slot's
                        memcpy(dst + len, in.data() + in_at + mb.in_off, mb.in_len);
                        mb.in_off = (uint32_t)len;
                        mb.out_off = (uint32_t)text;
                        dir_end[-(ptrdiff_t)(nm + 1u)] = mb;
                        len += mb.in_len;
                        text += mb.isize;
                        nm++;
                        in_at += msize;
                        if (text >= chunk) break;
                        continue;
                    }
                    if (st == 1 && !in_eof) {  // a member cut by a read boundary: more bytes
                        memmove(in.data(), in.data() + in_at, in_len - in_at);
                        in_len -= in_at;
                        in_at = 0;
                        const ssize_t got = raw_read(in.data() + in_len, in.size() - in_len);
                        if (got < 0) { bad = true; break; }
                        if (got == 0) in_eof = true;
                        in_len += (size_t)got;
                        continue;
                    }
                    if (in_at == in_len) at_end = true;  // the end of the file, after a whole member
                    else to_zlib = true;                 // not BGZF, or a member the end of the file cut: zlib says what it is
                    break;
                }
                if (to_zlib) {
                    mode = M_ZLIB;
                    zs.next_in = in.data() + in_at;
                    zs.avail_in = (uInt)(in_len - in_at);
                    if (!nm) continue;  // (nothing for the device in this slot: the zlib loop fills it)
                }
                at_end = at_end || bad || (!to_zlib && in_eof && in_at == in_len);
                text_bytes += text;
                publish(len, at_end, true, nm, text);
                continue;
            }
            if (mode == M_PLAIN || mode == M_GZRAW) {
                const size_t now = std::min(chunk, in_len - plain_at);
                memcpy(dst, in.data() + plain_at, now);
                plain_at += now;
                len = now;
                while (len < chunk && !in_eof) {
                    const ssize_t got = raw_read(dst + len, chunk - len);
                    if (got < 0) { bad = true; break; }
                    if (got == 0) in_eof = true;
                    len += (size_t)got;
                }
                at_end = bad || (in_eof && plain_at == in_len);
            } else {
                int rc = Z_OK;
                while (len < chunk) {
                    if (zs.avail_in == 0 && !in_eof) {
                        const ssize_t got = raw_read(in.data(), in.size());
                        if (got < 0) { bad = true; break; }
                        if (got == 0) in_eof = true;
                        zs.next_in = in.data();
                        zs.avail_in = (uInt)got;
                    }
                    zs.next_out = dst + len;
                    zs.avail_out = (uInt)(chunk - len);
                    rc = inflate(&zs, Z_NO_FLUSH);
                    len = chunk - zs.avail_out;
                    if (rc == Z_STREAM_END) {
                        members_host++;
                        if (zs.avail_in == 0 && !in_eof) {  // more members may follow: look
                            const ssize_t got = raw_read(in.data(), in.size());
                            if (got < 0) { bad = true; break; }
                            if (got == 0) in_eof = true;
                            zs.next_in = in.data();
                            zs.avail_in = (uInt)got;
                        }
                        if (zs.avail_in == 0 && in_eof) { at_end = true; break; }
                        if (inflateReset(&zs) != Z_OK) { rc = Z_DATA_ERROR; }
                        else continue;  // next member
                    }
                    if (rc == Z_OK || (rc == Z_BUF_ERROR && (zs.avail_out == 0 || (zs.avail_in == 0 && !in_eof)))) {
                        if (zs.avail_in == 0 && in_eof && zs.avail_out != 0) rc = Z_DATA_ERROR;  // truncated stream
                        else continue;
                    }
                    if (rc == Z_BUF_ERROR) rc = Z_DATA_ERROR;  // (no progress with all input consumed: truncated)
                    char code[16];
                    snprintf(code, sizeof code, "%d", rc);
                    fail(VS_E_ARG, "%s: not a complete gzip stream (zlib code %s)", path.c_str(), code);
                    bad = true;
                    break;
                }
                at_end = at_end || bad;
            }
            if (mode != M_GZRAW) text_bytes += len;
            publish(len, at_end, false, 0, 0, mode == M_GZRAW);
        }
        if (zs_open) inflateEnd(&zs);
    }
    void publish(size_t len, bool last, bool comp = false, uint32_t n_members = 0, size_t text = 0, bool gz = false) {
        std::lock_guard<std::mutex> lk(m);
        Slot &s = slots[filled % STREAM_RING_SLOTS];
        s.len = len;
        s.last = last;
        s.comp = comp;
        s.n_members = n_members;
        s.gz = gz;
        s.text = comp ? text : gz ? 0 : len;
        filled++;
        finished = last;
        cv.notify_all();
    }
    // the next filled slot (blocks until the reader has one)
    Slot &take() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return filled > taken; });
        return slots[taken % STREAM_RING_SLOTS];
    }
    void give_back() {
        std::lock_guard<std::mutex> lk(m);
        taken++;
        cv.notify_all();
    }
    void shut() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
        for (Slot &s : slots) s.buf.reset();
        if (fd >= 0) close(fd);
        fd = -1;
    }
};

// The open-time switches of a FASTQ stream, for the reader of one of its files: VS_BGZF_DEVICE=0 (BGZF through zlib too),
// VS_GZIP_DEVICE=1 (plain gzip decoded on the device; never for a member range, which is BGZF's) and VS_GZIP_TEXT (tests only, as
// VS_STREAM_CHUNK: the text a gzip round may add, for the window's GzStream::text_cap)
inline void fastq_switches(Reader &r, bool ranged, uint32_t &gz_text_cap) {
    if (const char *ev = getenv("VS_BGZF_DEVICE")) r.bgzf_device = strcmp(ev, "0") != 0;
    if (const char *ev = getenv("VS_GZIP_DEVICE")) r.gzip_device = !ranged && strcmp(ev, "1") == 0;
    if (const char *ev = getenv("VS_GZIP_TEXT")) gz_text_cap = (uint32_t)std::max<long long>(1, atoll(ev));
}

// What every stream keeps beside its readers: the status words its kernels write and the pinned copy the host reads, and how
// the stream ended.  A stream that has failed stays failed: every later call reports the stored failure again.
struct StreamState {
    VsDevBuf stat_buf;
    VsPinnedBuf h_stat_buf;
    uint32_t *d_stat = nullptr, *h_stat = nullptr;  // `words` words each, in the two buffers above
    bool done = false;
    int failed = VS_OK;
    std::string failed_msg;

    hipError_t reserve_stat(uint32_t words) {  // both zeroed
        hipError_t e = stat_buf.reserve(sizeof(uint32_t) * words);
        if (e == hipSuccess) e = h_stat_buf.reserve(sizeof(uint32_t) * words);
        if (e != hipSuccess) return e;
        d_stat = stat_buf.as<uint32_t>();
        h_stat = h_stat_buf.as<uint32_t>();
        memset(h_stat, 0, sizeof(uint32_t) * words);
        return hipMemset(d_stat, 0, sizeof(uint32_t) * words);
    }
    int fail(vs_ctx *ctx, int code, const std::string &msg) {
        done = true;
        failed = code;
        failed_msg = msg;
        return again(ctx);
    }
    int again(vs_ctx *ctx) const {
        if (ctx) ctx->err = failed_msg;  // (whole: two paths and two header lines of 200 bytes do not fit the formatting buffer of vs_fail)
        return failed;
    }
    // a block that could not be built in entry `who`
    int fail_hip(vs_ctx *ctx, const char *who, hipError_t e) {
        if (e == hipErrorOutOfMemory) return fail(ctx, VS_E_OOM, std::string(who) + ": device buffers for the block");
        return fail(ctx, VS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
};

// the refusal of a FASTQ record (numbered in file order) whose end the block builder found over the limit (VS_BLK_OVER)
inline std::string too_long_line(const std::string &path, uint64_t record) {
    return path + ": record " + std::to_string(record) + " has a sequence line of more than " + std::to_string((unsigned)VS_LEN_MASK) + " bytes";
}
// ... where the record's index in the window is on the device, in a list (0 if it cannot be fetched)
inline uint32_t fetch_u32(const uint32_t *d) {
    uint32_t v = 0;
    return hipMemcpy(&v, d, sizeof v, hipMemcpyDeviceToHost) == hipSuccess ? v : 0u;
}

// A taken slot: the reader's next filled slot (the constructor blocks until there is one), given back when the lease ends or
// is moved over -- by then the holder has seen to it that the slot's bytes are on the device.
struct SlotLease {
    SlotLease() = default;
    explicit SlotLease(Reader &r) : rd(&r), slot(&r.take()) {}
    SlotLease(SlotLease &&o) noexcept : rd(o.rd), slot(o.slot) { o.rd = nullptr, o.slot = nullptr; }
    SlotLease &operator=(SlotLease &&o) noexcept {
        if (this != &o) {
            give_back();
            rd = o.rd, slot = o.slot;
            o.rd = nullptr, o.slot = nullptr;
        }
        return *this;
    }
    ~SlotLease() { give_back(); }
    void give_back() {
        if (rd) rd->give_back();
        rd = nullptr, slot = nullptr;
    }
    explicit operator bool() const { return slot != nullptr; }
    const Slot &operator*() const { return *slot; }
    const Slot *operator->() const { return slot; }

private:
    Reader *rd = nullptr;
    Slot *slot = nullptr;
};

// room for `need` elements of T, a quarter more when the buffer has to grow (what it held is not kept)
template <typename T>
int reserve_n(vs_ctx *ctx, VsDevBuf &b, size_t need) {
    VS_HIP(ctx, b.reserve(need * sizeof(T), (need + need / 4 + 64) * sizeof(T)));
    return VS_OK;
}

}  // namespace
