// The device window of the streamed ingests (vs_stream.hip: one per FASTQ file; vs_bam.hip: the BAM stream and the share
// summary): the bytes left over from the last block + the reader's slots appended since, in one of two buffers.
//
// What holds for every window, written here once:
//  * Padding.  buf[cur] holds at least padded(size) = size rounded up to 16, + 16 bytes.  The line scanner (sl_load16) and
//    the BAM chain read whole 16-byte words, the last of which runs past `size`; the bytes beyond `size` are never meant.
//  * Growth.  A buffer that has to grow gets a quarter more than was asked for (reserve_n), and what it held is not kept:
//    the window's bytes are therefore never grown in place but copied to the OTHER buffer, which becomes the current one.
//  * make_room, keep_from and other may free and reallocate the buffer that is NOT current.  Whoever calls them has
//    synchronised the stream since the last operation that read or wrote that buffer -- the copy of an earlier keep_from or
//    make_room out of it, a kernel that was given data() before the flip.  (hipFree waits for the device, so a caller that
//    has not is slower, not wrong; the type itself adds no wait.)
//  * A slot may go back to the reader only after its bytes are on the device: append enqueues the uploads and returns, the
//    caller synchronises the stream before the lease ends.  append_members alone synchronises, because the directory it
//    uploads lives only for the call.
//  * The limit.  size never passes STREAM_MAX_WINDOW (offsets into a window are 32-bit).  The callers check that before they
//    append and word it for their input; an append beyond it is a programming error here (VS_E_STATE).
#pragma once
#include "vs_gzip_stream.h"
#include "vs_stream_reader.h"

namespace {

struct DevWindow {
    VsDevBuf buf[2];  // bytes
    int cur = 0;
    size_t size = 0;  // [0, size) of buf[cur] is the window
    // BGZF: the device copy of a slot's payloads and directory, a status word per member; members inflated so far
    VsDevBuf comp, dir, mstat;  // bytes, vs_bgzf_member, uint32
    uint64_t members = 0;
    // plain gzip inflated on the device (VS_GZIP_DEVICE=1): what goes from one window of the file to the next
    GzStream gz;
    uint32_t gz_status = 0;  // the status word with which the file's gzip stream failed, 0: it has not

    static size_t padded(size_t n) { return ((n + 15u) & ~(size_t)15u) + 16u; }
    uint8_t *data() { return buf[cur].as<uint8_t>(); }
    const uint8_t *data() const { return buf[cur].as<const uint8_t>(); }

    // room for a window of `need` bytes in the buffer that is not current (what that buffer held is gone); flip makes it the window
    int other(vs_ctx *ctx, size_t need, uint8_t **dst) {
        if (int rc = reserve_n<uint8_t>(ctx, buf[cur ^ 1], padded(need))) return rc;
        *dst = buf[cur ^ 1].as<uint8_t>();
        return VS_OK;
    }
    void flip(size_t new_size) {
        cur ^= 1;
        size = new_size;
    }
    // capacity for size + extra bytes, the window kept: in place, or copied to the other buffer once that has grown
    int make_room(vs_ctx *ctx, hipStream_t st, size_t extra) {
        if (size + extra > STREAM_MAX_WINDOW) return vs_fail(ctx, VS_E_STATE, "a window of %llu bytes", (unsigned long long)(size + extra));
        if (buf[cur].capacity() >= padded(size + extra)) return VS_OK;
        uint8_t *dst = nullptr;
        if (int rc = other(ctx, size + extra, &dst)) return rc;
        if (size) VS_HIP(ctx, hipMemcpyAsync(dst, data(), size, hipMemcpyDeviceToDevice, st));
        flip(size);
        return VS_OK;
    }
    // the window without its first `cut` bytes: the rest to the front of the other buffer
    int keep_from(vs_ctx *ctx, hipStream_t st, size_t cut) {
        const size_t rest = size - cut;
        uint8_t *dst = nullptr;
        if (int rc = other(ctx, rest, &dst)) return rc;
        if (rest) VS_HIP(ctx, hipMemcpyAsync(dst, data() + cut, rest, hipMemcpyDeviceToDevice, st));
        flip(rest);
        return VS_OK;
    }
    // the payloads of a BGZF slot to the device (once per slot, before its members are inflated)
    int upload_payloads(vs_ctx *ctx, hipStream_t st, const Slot &sl) {
        if (int rc = reserve_n<uint8_t>(ctx, comp, sl.len + 16u)) return rc;
        if (sl.len) VS_HIP(ctx, hipMemcpyAsync(comp.as<uint8_t>(), sl.buf.as<uint8_t>(), sl.len, hipMemcpyHostToDevice, st));
        return VS_OK;
    }
    // A whole slot appended: its text uploaded, or its BGZF members uploaded and inflated behind `size`.  *first_bad (device)
    // gets base + the index of the first member that does not inflate to its CRC32 and size, if there is one.
    int append(vs_ctx *ctx, hipStream_t st, const Slot &sl, uint32_t *first_bad, uint32_t base) {
        if (int rc = make_room(ctx, st, sl.text)) return rc;
        if (sl.comp) {
            const uint32_t nm = sl.n_members;
            if (!nm) return VS_OK;
            if (int rc = upload_payloads(ctx, st, sl)) return rc;
            return inflate_behind(ctx, st, sl.len, &slot_member(sl, nm - 1u), nm, sl.text, 1, first_bad, base);  // (the slot's own directory: the last member first)
        }
        if (sl.len) VS_HIP(ctx, hipMemcpyAsync(data() + size, sl.buf.as<uint8_t>(), sl.len, hipMemcpyHostToDevice, st));
        size += sl.text;
        return VS_OK;
    }
    // A slot of a plain gzip file (sl.gz) appended: uploaded, its block starts found, the runs counted and chained, decoded to
    // symbols, the histories handed down, the symbols resolved to text behind `size` (vs_gz_window); what could not finish
    // inside the slot is carried.  Synchronises the stream.  A stream that fails leaves its status word in gz_status and the
    // window as it was; the caller words it.  limit_msg: the path for the message of a window beyond STREAM_MAX_WINDOW.
    int append_gzip(vs_ctx *ctx, hipStream_t st, const Slot *sl, const char *limit_msg) {
        const std::function<int(size_t, uint8_t **)> room = [&](size_t text, uint8_t **dst) -> int {
            if (size + text > STREAM_MAX_WINDOW)
                return vs_fail(ctx, VS_E_RANGE, "%s: a window of %llu bytes without a complete record", limit_msg, (unsigned long long)(size + text));
            if (int rc = make_room(ctx, st, text)) return rc;
            *dst = data() + size;
            return VS_OK;
        };
        // sl == nullptr: a round on what is pending (gz.more: the cap of the round before held whole runs back)
        size_t text = 0;
        if (int rc = vs_gz_window(ctx, st, gz, sl ? sl->buf.as<uint8_t>() : nullptr, sl ? sl->len : 0, sl ? sl->last : gz.last_seen, room, &text, &gz_status))
            return rc;
        size += text;
        if (gz_status) gz.more = false;
        if (!gz_status && gz.last_seen && !gz.more && !(gz.at_member && gz.pend.empty())) gz_status = 8u;  // INF_E_INPUT: the file ends inside a member
        return VS_OK;
    }
    // the file's end is reached: its last slot has been appended and nothing decodable is pending
    bool gzip_at_end() const { return gz.last_seen && !gz.more; }
    // Members [a, b) of a BGZF slot whose payloads are uploaded, inflated behind `size` (a forward directory, out_off from 0).
    // Synchronises the stream: the directory of the sub-range is made here and read by the upload.
    int append_members(vs_ctx *ctx, hipStream_t st, const Slot &sl, uint32_t a, uint32_t b, uint32_t *first_bad, uint32_t base) {
        std::vector<vs_bgzf_member> sub;
        uint64_t text = 0;
        for (uint32_t i = a; i < b; i++) {
            vs_bgzf_member m = slot_member(sl, i);
            m.out_off = (uint32_t)text;
            text += m.isize;
            sub.push_back(m);
        }
        if (int rc = make_room(ctx, st, text)) return rc;
        if (int rc = inflate_behind(ctx, st, sl.len, sub.data(), b - a, text, 0, first_bad, base)) return rc;
        VS_HIP(ctx, hipStreamSynchronize(st));
        return VS_OK;
    }

private:
    // n members of comp[0, comp_len), their directory at host_dir, inflated to the `text` bytes behind `size`
    int inflate_behind(vs_ctx *ctx, hipStream_t st, size_t comp_len, const vs_bgzf_member *host_dir, uint32_t n, size_t text, int reversed,
                       uint32_t *first_bad, uint32_t base) {
        if (int rc = reserve_n<vs_bgzf_member>(ctx, dir, (size_t)n)) return rc;
        if (int rc = reserve_n<uint32_t>(ctx, mstat, (size_t)n)) return rc;
        VS_HIP(ctx, hipMemcpyAsync(dir.as<vs_bgzf_member>(), host_dir, sizeof(vs_bgzf_member) * n, hipMemcpyHostToDevice, st));
        vs_launch_inflate(st, comp.as<uint8_t>(), comp_len, data() + size, text, dir.as<vs_bgzf_member>(), n, mstat.as<uint32_t>(), first_bad, base, reversed);
        VS_HIP(ctx, hipGetLastError());
        members += n;
        size += text;
        return VS_OK;
    }
};

}  // namespace
