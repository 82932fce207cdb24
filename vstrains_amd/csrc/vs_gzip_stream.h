// What the streamed ingest keeps per plain gzip file between two windows of it (vs_gz_window of vs_gzip.hip), and the device
// buffers the windows share.  Host code only.
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "vs_buf.h"

struct vs_ctx;

struct GzDev {  // grow-only, reused from window to window
    VsDevBuf comp, count, list, starts, res, chain, sym, mem, hist, seg, status;
};

struct GzStream {
    GzDev dev;
    VsDevBuf hist0;             // the resolved last 32 KiB of text (device)
    std::vector<uint8_t> pend;  // compressed bytes not yet decoded: from the byte in which the next run starts
    uint32_t bit = 0;           // that run's bit offset from pend[0]
    bool at_member = true;      // pend starts with a member header (the start of the file, behind a trailer), no run
    uint32_t valid = 0;         // bytes of hist0 that belong to the open member
    uint32_t crc = 0;           // the open member's CRC32 and length so far
    uint64_t bytes = 0;
    uint64_t windows = 0, runs = 0, dropped = 0, members = 0, text = 0, recounted = 0;
    uint32_t text_cap = 1u << 30;  // text of one round: its 16-bit symbols and its bytes stay below the window limit
                                   // (VS_GZIP_TEXT overrides it: tests only, several capped rounds of a small file)
    bool more = false;      // the cap held back whole runs that lie in pend: the next round decodes them before a slot is taken
    bool last_seen = false; // the file's last piece is in pend (or decoded)
};

#define GZ_STREAM_GRAN 16384u       // compressed bytes per selected start in the streamed ingest

// One more piece data[0, n) of the file (last: its end; n = 0 while g.more: a round on what is pending) through the kernels.  `room` is asked once for the address of
// `text` more bytes behind the window; *text = what was appended (0: the piece ended inside the first run, more is needed).
// *status = 0, or the status word (vs_gzip_core.h) with which the stream has failed.  VS_E_RANGE when one run does not fit.
int vs_gz_window(vs_ctx *ctx, hipStream_t st, GzStream &g, const uint8_t *data, size_t n, bool last,
                 const std::function<int(size_t, uint8_t **)> &room, size_t *text, uint32_t *status);
const char *vs_gz_status_name(uint32_t status);
