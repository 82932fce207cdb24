/*
 * vstrains_hip.h -- C ABI of libvstrains_hip.so, the MI355X (gfx950) implementation of the
 * VStrains hot path.  extern "C", plain pointers and sizes only; no C++ or torch types cross
 * this line.  Host code (Python via ctypes, or any C caller) binds exactly these symbols.
 *
 * Every entry returns 0 on success and a negative VS_E_* code on failure; the message is
 * available from vs_last_error(ctx) (or vs_last_error(NULL) for vs_ctx_create failures).
 * A context belongs to one device and one host thread at a time.  Nothing here falls back
 * to the CPU: without a usable HIP device the calls fail with VS_E_HIP.
 *
 * "Replaces" cites the reference lines (under /root/reference/) each entry stands in for.
 */
#ifndef VSTRAINS_HIP_H
#define VSTRAINS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_ABI_VERSION 11

enum {
    VS_OK = 0,
    VS_E_ARG = -1,       /* bad argument */
    VS_E_HIP = -2,       /* HIP runtime error (no device, launch failure, ...) */
    VS_E_OOM = -3,       /* device or host allocation failed */
    VS_E_NODE_BASE = -4, /* a node of length >= k+1 holds a byte outside ACGT: the reference
                            dies with KeyError in reverse_seq (PE_Inference.py:12-13,122) */
    VS_E_STATE = -5,     /* call order (e.g. counting before an index exists) */
    VS_E_RANGE = -6,     /* a size exceeds what this build supports */
    VS_E_UTF8 = -7,      /* a FASTQ sequence line holds bytes that are not valid UTF-8: the reference's
                            text-mode readlines() raises UnicodeDecodeError (PE_Inference.py:147-152) */
    VS_E_KEY = -8,       /* a graph stage looked up an id / index that is not there: the reference raises
                            KeyError / IndexError / ValueError at that point (vs_stage_error names which) */
    VS_E_FPE = -9,       /* an edge flow would divide by a zero neighbour sum: FloatingPointError under the
                            reference's numpy.seterr(all="raise") (vstrains:25, Utilities.py:20-30) */
    VS_E_RECURSION = -10 /* (ABI 8) a chain of forked ids is longer than the reference's recursive merge_id
                            (Utilities.py:318-327) can follow under CPython's recursion limit: the reference
                            ends with RecursionError there (runaway trivial splits on circular graphs) */
};

typedef struct vs_ctx vs_ctx;     /* one per device */
typedef struct vs_reads vs_reads; /* a device-resident block of packed read pairs */

/* ---- context ------------------------------------------------------------------------------ */
int vs_abi_version(void);
int vs_device_count(void);
int vs_ctx_create(int device, vs_ctx **out);
void vs_ctx_destroy(vs_ctx *ctx);
const char *vs_last_error(const vs_ctx *ctx);
/* Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream). */
int vs_ctx_set_stream(vs_ctx *ctx, void *stream);
int vs_ctx_sync(vs_ctx *ctx);

/* ---- K1: node index -------------------------------------------------------------------------
 * Replaces utils/VStrains_PE_Inference.py:114-135 (split_len = k+1; the dict of every
 * (k+1)-mer window of every node, forward and reverse-complemented).
 * node_ascii: the N node sequences concatenated (host memory); node_off[N+1]: byte offsets.
 * On VS_E_NODE_BASE, bad_node / bad_char (may be NULL) receive the node index and the byte the
 * reference's KeyError would name.  Rebuilding replaces the previous index. */
int vs_index_build(vs_ctx *ctx, const uint8_t *node_ascii, const uint64_t *node_off,
                   uint32_t n_nodes, uint32_t ksize, uint32_t *bad_node, uint8_t *bad_char);

/* Index facts for reporting: info[0]=seed length w, [1]=probe stride s, [2]=seed positions
 * indexed, [3]=hash slots, [4]=distinct seeds, [5]=bytes of device memory held by the index. */
int vs_index_info(const vs_ctx *ctx, uint64_t info[6]);

/* Testing aid: the index the context holds, copied to host memory as the kernels read it (no kernel runs, nothing on
 * the counting path changes).  sizes[0]=hash slots, [1]=postings (= seed positions), [2]=packed words per strand
 * INCLUDING the zero pad words behind the text, [3]=nodes, [4]=log2 of the slots.  Every buffer may be NULL (not copied;
 * call once with all NULL for the sizes): slots[sizes[0]] of 16 B (key u64 | a u32 | b u32), postings[sizes[1]] of 16 B
 * (node | pos + strand << 31 | node length | first word), fwd_words / rc_words[sizes[2]], meta[sizes[3]] of 8 B
 * (first word | length). */
int vs_index_export(vs_ctx *ctx, void *slots, void *postings, uint32_t *fwd_words, uint32_t *rc_words, void *meta,
                    uint64_t sizes[5]);

/* A numbering of the nodes that runs along the graph's paths (host only; depth-first over k-base overlaps, either strand).
 * order_out[n_nodes]: order_out[r] = the node (position in node_off) that should be handed to vs_index_build as number r.
 * Optional, for speed only: the matrices vs_pe_count fills are indexed by the numbering vs_index_build was given
 * (PE_Inference.py:139-140 indexes them by GFA position), and every result is the same sum under any numbering -- but
 * pairs are processed in the order of the node their forward read starts in, a slice per XCD, and a numbering that
 * scatters the neighbours of a path costs 20-25 % of the step (csrc/vs_order_host.cpp).  The Python host side does this
 * by default and maps the matrices back (vstrains_amd/pe.py). */
int vs_node_order_host(const uint8_t *node_ascii, const uint64_t *node_off, uint32_t n_nodes, uint32_t ksize,
                       uint32_t *order_out);

/* ---- read blocks ----------------------------------------------------------------------------
 * Replaces the FASTQ record slicing of PE_Inference.py:146-159 from the point where the two
 * sequence strings of a pair are known.  Ends are interleaved: end 2r = forward read of pair
 * r, end 2r+1 = its reverse read.  ascii/off are host memory: off[n_ends+1] byte offsets into
 * ascii.  Bytes are taken verbatim: 'N' marks the pair as an N-pair (:160); any other byte
 * outside ACGT makes every window covering it miss, as a dict lookup would (:25-26). */
int vs_reads_pack(vs_ctx *ctx, const uint8_t *ascii, const uint64_t *off, uint64_t n_ends,
                  vs_reads **out);
void vs_reads_free(vs_ctx *ctx, vs_reads *reads);
/* info[0]=ends, [1]=packed words, [2]=max read length, [3]=ends holding bytes outside ACGTN,
 * [4]=device bytes held. */
int vs_reads_info(const vs_reads *reads, uint64_t info[5]);
/* Unpack back to ASCII (ACGT only; testing aid).  out must hold off[n_ends] bytes where off is
 * the cumulative read length; lens[n_ends] and flags[n_ends] (bit0: has N, bit1: has other
 * non-ACGT) may be NULL. */
int vs_reads_unpack(vs_ctx *ctx, const vs_reads *reads, uint8_t *out, uint32_t *lens,
                    uint8_t *flags);
/* Unpaired reads (additions to ABI 11 without a new number: nothing that exists changes): a SINGLES BLOCK of n reads is a block of 2n ends in which
 * end 2r is read r and end 2r+1 is absent (length 0, no words, flag bit 3).  The counting kernels treat read r as the
 * reference treats ONE end of a pair (PE_Inference.py:160-184 restricted to one end): a read with an 'N' is counted as an
 * N read and nothing else; otherwise one shorter than k+1 as a short read and nothing else; otherwise it is used:
 * short_mat[L[a]][L[b]] += 1 for a <= b over its accepted nodes L.  node_mat is never touched.  The three words vs_pe_count
 * adds to `stats` are then tallies of READS (with N, short, used): hand it a stats array of its own to keep them apart
 * from the pairs'.  A block spends one empty end slot per read (8 bytes).
 *   vs_reads_pack_single : as vs_reads_pack from host text, off[n_reads + 1], one read per slot; vs_reads_info says
 *                          ends = 2 n_reads, vs_reads_unpack returns the absent ends with length 0 (flags bit 3 set)
 *   vs_reads_unpaired    : 1 for a singles block, 0 for a block of pairs (all slots of a block are one or the other) */
int vs_reads_pack_single(vs_ctx *ctx, const uint8_t *ascii, const uint64_t *off, uint64_t n_reads, vs_reads **out);
int vs_reads_unpaired(const vs_reads *reads);

/* ---- FASTQ ingest (host, multi-threaded) -----------------------------------------------------
 * Replaces PE_Inference.py:146-159: both files read in text mode (universal newlines), record r
 * = lines 4r..4r+3, sequence = line 4r+1 minus its last character (the newline, or a real
 * character on a final line without one), n_pairs = min(lines_f // 4, lines_r // 4).  Text mode means
 * the reference sees CHARACTERS: a valid UTF-8 multi-byte sequence inside a sequence line is one character
 * (counted once, every window over it misses); vs_fastq_sequence / _gather / _block deliver one byte per
 * character ('?' for a multi-byte one); invalid UTF-8 there is VS_E_UTF8.
 * vs_fastq_open maps and indexes both files on the host cores (VS_HOST_THREADS overrides the
 * count); a file that starts with the gzip magic is inflated into memory first (zlib; several
 * members in a row are fine, a cut-off stream is VS_E_ARG).  vs_fastq_block turns pairs
 * [first, first+count) into a device read block. */
/* The host packer the ingest uses on every sequence line: `len` bytes -> ceil(len/16) words, 16
 * bases per word, LSB first, A C G T = 0 1 2 3, any other byte packs as 0; *flags: bit 0 an 'N',
 * bit 1 another ASCII byte outside ACGT, bit 7 a byte >= 0x80.  plain != 0 takes the byte-by-byte
 * body instead of the vector one (same result; tests compare the two). */
int vs_pack_sequence(const uint8_t *seq, uint32_t len, uint32_t *words, uint32_t *flags, int plain);
typedef struct vs_fastq vs_fastq;
int vs_fastq_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, vs_fastq **out);
void vs_fastq_close(vs_fastq *fq);
/* Cooperative open for one process per GPU, so that no rank reads a whole file (PE_Inference.py:146-154 reads both
 * files completely; its total = min(lines_f // 4, lines_r // 4) follows from the ranks' counts):
 *   1. every rank r calls vs_fastq_count_part(path, r, world, out) for both files: out[0] = newlines in its byte
 *      range, out[1] = file size, out[2] = flags (bit 0: the range holds '\r', bit 1: gzip file, bit 2: the file does
 *      not end in a newline); the ranks exchange these (an all-gather of three integers per file);
 *   2. from the totals every rank derives its record range and calls vs_fastq_open_records with everybody's counts:
 *      only the bytes of records [first, last) are indexed; the handle numbers them from 0.
 * Files with '\r' or gzip files are opened whole (vs_fastq_open) by every rank instead -- except a pair of whole BGZF files
 * of plain ASCII with LF line ends, which the ranks share by MEMBER and inflate on their devices (the member-sharded open
 * further down: vs_bgzf_walk_file .. vs_fastq_stream_open_range). */
int vs_fastq_count_part(const char *path, uint32_t part, uint32_t n_parts, uint64_t out[3]);
int vs_fastq_open_records(vs_ctx *ctx, const char *fwd_path, const char *rve_path, uint32_t n_parts,
                          const uint64_t *counts_f, const uint64_t *counts_r, uint64_t first, uint64_t last,
                          vs_fastq **out);
/* text bytes the handle went through when it was opened (both files) */
uint64_t vs_fastq_bytes_indexed(const vs_fastq *fq);
/* info[0] = pairs, [1] = lines of the forward file, [2] = lines of the reverse file */
int vs_fastq_info(const vs_fastq *fq, uint64_t info[3]);
int vs_fastq_sequence(const vs_fastq *fq, int which, uint64_t record, uint8_t *buf, uint32_t cap,
                      uint32_t *len);
/* off[2*count+1] byte offsets of the interleaved ends (2r forward, 2r+1 reverse); ascii (may be
 * NULL to get the sizes only) receives the bytes.  Host pointers. */
int vs_fastq_gather(const vs_fastq *fq, uint64_t first, uint64_t count, uint64_t *off,
                    uint8_t *ascii);
int vs_fastq_block(vs_ctx *ctx, vs_fastq *fq, uint64_t first, uint64_t count, vs_reads **out);

/* Streamed ingest (additions to ABI 10): the same records from any file descriptor -- a FIFO, /dev/stdin, a process
 * substitution, a regular file -- read front to back through a bounded ring of pinned chunks (one reader thread per
 * file; gzip inflated on the fly, several members in a row are fine), the records found and packed on the device.  Peak
 * host memory is the ring, whatever the size of the input.
 *   vs_fastq_stream_open  : opens both files and starts their readers
 *   vs_fastq_stream_next  : the next block of at most max_pairs pairs (0 = no limit), the layout vs_pe_count takes, ready
 *                           when the call returns; *n_pairs = 0 and *out = NULL at the end of the input.  Before it reports
 *                           the end both files have been read to their ends: bytes that are not valid UTF-8 anywhere in
 *                           either file are VS_E_UTF8, a cut-off gzip stream VS_E_ARG (the first failure in file order, as
 *                           vs_fastq_open).  After a failure every call returns it again.
 *   vs_fastq_stream_info  : info[0] = pairs so far, [1] = text bytes read (inflated), [2] = file bytes read (compressed),
 *                           [3] = flags: bit 0 some chunk held '\r', bit 1 a byte >= 0x80, bit 2 / 3 the forward / reverse
 *                           file is gzip, bit 4 the end of the input was reported
 *   vs_fastq_stream_close : stops the readers and frees everything (blocks returned earlier stay valid)
 * VS_STREAM_CHUNK (bytes) overrides the chunk size: tests only, to put record and line boundaries across chunks. */
typedef struct vs_fastq_stream vs_fastq_stream;
int vs_fastq_stream_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, vs_fastq_stream **out);
int vs_fastq_stream_next(vs_ctx *ctx, vs_fastq_stream *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs);
int vs_fastq_stream_info(const vs_fastq_stream *s, uint64_t info[4]);
void vs_fastq_stream_close(vs_fastq_stream *s);
/* Test aid: the streamed ingest's device line scanner on n bytes of host text.  ends[i] (up to cap of them) = byte offset
 * of newline i; info[0] = newlines, [1] = flags (bit 0 '\r', bit 1 a byte >= 0x80), [2] = one past the newline of the last
 * line that completes a record when the text's first line has number line0 (lines 4r .. 4r+3 are record r), 0 if none. */
int vs_fastq_scan_text(vs_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t line0, uint64_t *ends, uint64_t cap,
                       uint64_t info[3]);

/* BGZF (additions to ABI 10): the blocked gzip of bgzip / htslib / samtools.  The streamed ingest inflates the members of
 * such a file ON THE DEVICE (one wavefront per member, vs_inflate.hip) unless VS_BGZF_DEVICE=0; any other gzip member keeps
 * the host zlib loop, from that byte on for the rest of its file.
 *   vs_bgzf_walk    : host only.  The whole BGZF members at the front of buf[0, n): members[4i .. 4i+3] (up to cap members)
 *                     = payload offset, payload length, ISIZE, CRC32; info[0] = members found, [1] = the offset of the first
 *                     byte that is not part of one, [2] = what is there: 0 nothing (the range ends after a member), 1 bytes
 *                     that may become a member ("need more bytes"), 2 not BGZF (any other gzip member, any other bytes, other
 *                     FLG bits, CM != 8, no BC subfield, BSIZE too small for header and trailer, ISIZE > 65536)
 *   vs_inflate_host : host only.  One raw deflate payload through the decoder the kernel runs, lane loops serial:
 *                     *status = 0, or the first thing wrong: 1 block type 3, 2 stored LEN/NLEN, 3 over-subscribed and
 *                     4 incomplete code lengths, 5 invalid literal/length and 6 distance symbol, 7 distance beyond the
 *                     member's own output, 8 payload exhausted, 9 output beyond and 10 short of ISIZE, 11 CRC32 mismatch,
 *                     12 bad code-length section, 13 payload bytes behind the final block, 14 bad descriptor.  Nothing is
 *                     written outside out[0, isize).
 *   vs_inflate_bgzf : test aid.  n host bytes of whole members through the device kernel; member i's bytes at
 *                     out[sum over j < i of (ISIZE_j + guard)], followed by `guard` bytes that keep the value 0xA5;
 *                     status[i] as above; info[0] = members, [1] = bytes of out used (out == NULL: the sizes only)
 *   vs_fastq_stream_inflate_info : info[2f + 0] = members of file f inflated on the device, [2f + 1] = on the host */
int vs_bgzf_walk(const uint8_t *buf, uint64_t n, uint64_t *members, uint64_t cap, uint64_t info[3]);
int vs_inflate_host(const uint8_t *payload, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc, uint32_t *status);
int vs_inflate_bgzf(vs_ctx *ctx, const uint8_t *data, uint64_t n, uint8_t *out, uint64_t out_cap, uint32_t guard, uint32_t *status,
                    uint64_t status_cap, uint64_t info[2]);
int vs_fastq_stream_inflate_info(const vs_fastq_stream *s, uint64_t info[4]);

/* ---- plain gzip on the device: one deflate stream decoded by many wavefronts (vs_gzip.hip, vs_gzip_core.h) -------
 * A gzip file that is not BGZF has no member directory.  Its blocks are found speculatively (every bit offset is tested for
 * the header of a non-final dynamic block), runs are decoded from the selected starts into 16-bit symbols that name bytes
 * of the unknown 32 KiB in front of a run, the runs that the known first block's run reaches ("the chain") hand their
 * histories down, and the symbols are resolved into bytes; CRC32 and ISIZE of every member are checked.
 *   vs_gzip_inflate      : test aid.  data[0, n) (n <= 256 MiB), a whole gzip file of one or more members, through the
 *                          kernels.  gran = compressed bytes per selected start (>= 16), 0 = every candidate.  The text to
 *                          out[0, info[7]), followed by `guard` bytes that keep the value 0xA5 (out == NULL: the sizes
 *                          only); nothing is written when the status is not 0.  info[0] = candidates (offsets that passed
 *                          the full header check, of those the search looked at), [1] = selected starts, [2] = chain runs,
 *                          [3] = runs dropped, [4] = members, [5] = status, 0 or the first thing wrong: the words of
 *                          vs_inflate_host, 15 no gzip member header, 16 ISIZE mismatch, [6] = the failing run's place
 *                          in the chain, [7] = bytes of text, [8] = chain runs counted a second time: a counted run other than the
 *                          first may read 64 finder spans of input (64 KiB at least) and is then given up (17); if the chain
 *                          reaches such a run it is counted again without the bound
 *   vs_gzip_inflate_host : host only.  The same routines with one lane, step for step; out and info as above, no guard
 *   vs_fastq_stream_gzip_info : with VS_GZIP_DEVICE=1 in the environment at vs_fastq_stream_open, a file that starts with
 *                          the gzip magic and whose first member is not BGZF is not inflated by zlib: its bytes go to the
 *                          device slot by slot and through the kernels above, one start per 16 KiB of compressed bytes; what
 *                          cannot finish inside a slot (the compressed bytes of the open run, its bit offset, the last
 *                          32 KiB of text, the open member's CRC32 and length) is carried to the next.  info[4f + 0] =
 *                          windows of file f decoded so, [4f + 1] = chain runs, [4f + 2] = runs dropped, [4f + 3] = members.
 *                          Such members count neither in members_device nor in members_host of
 *                          vs_fastq_stream_inflate_info.  A stream the device refuses fails as the zlib loop fails: VS_E_ARG,
 *                          "<path>: not a complete gzip stream (zlib code <c>)" for a regular file, which zlib reads again
 *                          for the code; a pipe gets "(device status <NAME>)" in its place */
int vs_gzip_inflate(vs_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t gran, uint8_t *out, uint64_t out_cap, uint32_t guard, uint64_t info[9]);
int vs_gzip_inflate_host(const uint8_t *data, uint64_t n, uint32_t gran, uint8_t *out, uint64_t out_cap, uint64_t info[9]);
int vs_fastq_stream_gzip_info(const vs_fastq_stream *s, uint64_t info[8]);

/* BGZF written on the device (additions to ABI 10): the other half of the above.  A text is cut into members of at most
 * 0xFF00 bytes (bgzip's cut) and every member is made by ONE wavefront (k_deflate, vs_deflate.hip) through the encoder of
 * csrc/vs_deflate_core.h, which the host runs from the same text with one lane: the bytes are the same, for every text.
 * A member is the 18-byte BGZF header, ONE final deflate block -- the smallest of stored, fixed Huffman and dynamic Huffman,
 * sized before anything is emitted -- CRC32 and ISIZE.  LZ77 with matches of 3 .. 258 bytes at most 32768 back, greedy; no
 * member is larger than its text + 31 bytes (the stored form), so BSIZE never passes 65536.
 *   vs_deflate_host : host only.  text[0, n), n <= 0xFF00, as ONE member into out[0, cap): *size its bytes, *kind = 0 stored,
 *                     1 fixed, 2 dynamic.  VS_E_ARG for a longer text, VS_E_RANGE when the member does not fit (nothing is
 *                     written then); cap = n + 31 always suffices.
 *   vs_deflate_bgzf : test aid.  n host bytes cut into members of 0xFF00 through the device kernel, every member in a device
 *                     slot of its own followed by `guard` bytes that must keep the value 0xA5 (checked, as is the rest of the
 *                     slot behind the member: VS_E_STATE), then packed back to back on the device; out receives the members
 *                     and the 28-byte EOF member.  info[0] = members without the EOF member, [1] = bytes of out used,
 *                     [2] / [3] / [4] = members that came out stored / fixed / dynamic */
int vs_deflate_host(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *size, uint32_t *kind);
int vs_deflate_bgzf(vs_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t out_cap, uint32_t guard, uint64_t info[5]);

/* Member-sharded open of a BGZF pair for one process per GPU (additions to ABI 10): no rank inflates a whole file, nothing
 * is inflated on a host, and every rank streams exactly its own records.  Both files must be regular files made of whole
 * BGZF members from the first byte to the last.  Two passes with one exchange between them (pe.FastqStream.open_shard):
 *   1. every rank walks the member headers of both files (vs_bgzf_walk_file), takes the members [M r / W, M (r + 1) / W) of
 *      each and has the device count their lines (vs_bgzf_count_lines); the ranks all-gather the per-member counts, the OR
 *      of the flags and the last byte of the last non-empty member;
 *   2. from everybody's counts every rank derives the pair total min(lines_f // 4, lines_r // 4) (PE_Inference.py:154), its
 *      record range and, per file, where to start (vs_bgzf_shard_plan), and opens the streamed ingest on that member range
 *      (vs_fastq_stream_open_range).
 * A rank inflates its share twice (the text of pass 1 is not kept: its device memory does not grow with the file); a '\r' or
 * a byte >= 0x80 anywhere, or a file that is not whole BGZF, sends all ranks to the cooperative open above instead.
 *   vs_bgzf_walk_file   : host only, reads headers and trailers, no payload.  offsets[i] (up to cap entries) = file offset of
 *                         member i, and one more entry = one past the last member; info[0] = members, [1] = the offset of the
 *                         first byte that is not part of one, [2] = what is there (0 / 1 / 2 as vs_bgzf_walk: the file
 *                         qualifies only with 0), [3] = the file's size
 *   vs_bgzf_count_lines : members [0, n) at offsets[0 .. n] (n + 1 entries, a slice of the walk's) read -- those bytes only --
 *                         and inflated on the device, `grid` wavefronts looping over them with one 64 KiB region each
 *                         (k_inflate_count); counts[i] = newlines of member i; info[0] = flags (bit 0 a '\r', bit 1 a byte
 *                         >= 0x80), [1] = the last byte of the last non-empty member (256: all are empty), [2] = members
 *                         inflated, [3] = file bytes read.  CRC32 and every check of the streamed inflate hold; a member the
 *                         device rejects is VS_E_ARG, worded by zlib on the host as the streamed ingest words it
 *   vs_inflate_count_host : host only.  The count of the kernel through the same decoder text, one lane: res[0] = status (as
 *                         vs_inflate_host), [1] = newlines, [2] = flags, [3] = last byte (0 for an empty member)
 *   vs_bgzf_shard_plan  : host only, a pure function.  counts[n_members] of ONE file, no_final_newline = its last byte is no
 *                         '\n'; for the records [first, last) (record r = lines 4r .. 4r+3): plan[0] = the first member to
 *                         open, [1] = the lines to skip in front of it, [2] = one past the last member needed.  The first
 *                         member is the one that holds the newline in front of line 4 * first, so neighbouring ranks share
 *                         that one member and no other; an empty range opens nothing ({0, 0, 0})
 *   vs_fastq_stream_open_range : the streamed ingest on range[3f .. 3f+2] = {offset of the first member, offset one past the
 *                         last, lines to skip} of file f; it delivers n_pairs pairs and then reports the end.  The readers
 *                         seek to the first offset and never read at or beyond the second; a final line without a newline
 *                         counts only where the range ends at the end of the file */
int vs_bgzf_walk_file(const char *path, uint64_t *offsets, uint64_t cap, uint64_t info[4]);
int vs_bgzf_count_lines(vs_ctx *ctx, const char *path, const uint64_t *offsets, uint64_t n, uint32_t *counts, uint64_t info[4]);
int vs_inflate_count_host(const uint8_t *payload, uint32_t len, uint32_t isize, uint32_t crc, uint32_t res[4]);
int vs_bgzf_shard_plan(const uint32_t *counts, uint64_t n_members, int no_final_newline, uint64_t first, uint64_t last, uint64_t plan[3]);
int vs_fastq_stream_open_range(vs_ctx *ctx, const char *fwd_path, const char *rve_path, const uint64_t range[6], uint64_t n_pairs,
                               vs_fastq_stream **out);

/* Read pairs from ONE collated BAM file (additions to ABI 10): the BGZF members inflated on the device as for FASTQ, the
 * records found there by following the chain of block_size fields from the end of the header, the 4-bit bases packed by
 * the one packer.  The file stands for the FASTQ pair `samtools fastq -1 -2` would write: records with flag 0x100 or 0x800
 * are dropped, records that are not 0x1 with exactly one of 0x40 / 0x80 are dropped ("other"), the rest are taken two at
 * a time, each couple one 0x40 (the forward end) and one 0x80 record in either order; an end with 0x10 is reversed and
 * complemented.  Two firsts or two seconds in a couple, or an odd record at the end, are VS_E_ARG ("not collated").
 *   vs_bam_stream_open  : a regular file whose first BGZF member inflates to "BAM\1" (a FIFO or anything else: VS_E_ARG);
 *                         the header (text and references) is inflated on the host with zlib and skipped on the device
 *   vs_bam_stream_next  : as vs_fastq_stream_next; a record cut by the end of the file ("truncated record") and a record
 *                         whose block_size is below 32 or smaller than its own fields need (named by its number from 0 in
 *                         the file) are VS_E_ARG
 *   vs_bam_stream_info  : info[0] = pairs delivered, [1] = records seen, [2] = dropped for 0x100 / 0x800, [3] = dropped as
 *                         other, [4] = members inflated on the device, [5] = text bytes (inflated), [6] = file bytes read,
 *                         [7] = 1 once the end of the input has been reached
 *   vs_bam_stream_close : as vs_fastq_stream_close
 * VS_BAM_SEG (tests only, like VS_STREAM_CHUNK) sets the segment of the chain passes, 64 .. 12288 bytes.
 *
 * Test aids, the chain alone.  bytes[0, n) are inflated BAM bytes, a record starts at `skip`; seg = 0 is the default.
 * recs[4 i ..] for the i-th whole record on the chain (at most cap_recs are written): its offset, flag | class << 16
 * (class 0 first, 1 second, 2 dropped for 0x900, 3 other, 4 malformed), l_seq, the offset of its bases; ends[2 c], [2 c + 1]
 * (at most cap_ends entries) = the record indices of the forward and the reverse end of couple c.  info[0] = records,
 * [1] = records that take part, [2] = how the chain ended (0 at byte n, 1 in front of a record the window cuts, 2 at a
 * block_size < 32), [3] = where, [4] = index of the first malformed record, [5] = the first couple that is not one first
 * and one second (~0: none).  vs_bam_scan_host: the same text with one host thread; vs_bam_scan_text: the kernels. */
typedef struct vs_bam_stream vs_bam_stream;
int vs_bam_stream_open(vs_ctx *ctx, const char *path, vs_bam_stream **out);
int vs_bam_stream_next(vs_ctx *ctx, vs_bam_stream *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs);
int vs_bam_stream_info(const vs_bam_stream *s, uint64_t info[8]);
void vs_bam_stream_close(vs_bam_stream *s);
int vs_bam_scan_host(const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t *recs, uint64_t cap_recs, uint32_t *ends,
                     uint64_t cap_ends, uint64_t info[6]);
int vs_bam_scan_text(vs_ctx *ctx, const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t *recs, uint64_t cap_recs,
                     uint32_t *ends, uint64_t cap_ends, uint64_t info[6]);
/* Mates matched by name (additions to ABI 10): the participating records of ONE regular BAM in ANY record order -- a
 * coordinate-sorted alignment, `samtools view -f 12` of one, a file that lost one mate of some pairs.  The file stands for
 * the pair `samtools collate | samtools fastq -1 R1 -2 R2 -s /dev/null -0 /dev/null` writes, up to the order of the pairs
 * (no result depends on it).  The rule: records are walked in file order, classified as above, and only first and second
 * records take part.  The name of a record is its l_read_name bytes as they lie in it, terminator included; two names are
 * the same when lengths and bytes are (never because a hash is).  A record of class c pairs with the OLDEST waiting record
 * of its name and the other class, or waits when there is none: the j-th first of a name pairs with its j-th second, the
 * first is the forward end.  Pairs are delivered in the order of the record that completed them, whatever the window,
 * chunk, segment or block size.  What still waits at the end of the input are singletons: dropped and counted.
 *   vs_bam_stream_open_mode : mode VS_BAM_COLLATED is vs_bam_stream_open; VS_BAM_BY_NAME selects the above.  next, info
 *                             (info[0..7] keep their meaning) and close serve both.  Truncated and malformed records and
 *                             damaged members fail as in the collated mode.  VS_E_RANGE, with advice to run `samtools
 *                             collate`: more than 64 records of one name and one class in one window (the waiting ones
 *                             included; the newest record of the name is named -- this bounds every list walk), and
 *                             waiting records plus the next chunk beyond the largest window.
 *                             VS_BAM_BY_NAME_KEEP (an addition to ABI 11; the other modes unchanged, a member range takes
 *                             the collated mode only): matching, carrying, the cap of 64 per name and every refusal are those
 *                             of VS_BAM_BY_NAME, but the singletons are KEPT: at the end of the input the records that still
 *                             wait are handed out, in file order, as singles blocks (vs_reads_pack_single above has the
 *                             layout) of at most max_pairs slots.  End 2 r of such a block is the bases of waiting record r as
 *                             `samtools fastq -s` writes them (reversed and complemented under 0x10), end 2 r + 1 is absent;
 *                             a record with l_seq == 0 is a read of length 0, present and short.  *n_pairs of next is then
 *                             the number of SLOTS of the block and vs_reads_unpaired tells its kind.  No mixed block is made
 *   vs_bam_stream_mate_info : info[0] = singletons (dropped, or kept under VS_BAM_BY_NAME_KEEP), [1] = most records carried between two windows, [2] = most
 *                             bytes carried, [3] = windows scanned
 * VS_BAM_NAME_BITS=<0..64> (tests only) keeps that many low bits of the name hash: long probe chains without constructed
 * collisions.
 * Test aids, the match of one window: bytes, n, skip, seg as vs_bam_scan_*; hash_bits as VS_BAM_NAME_BITS.  pairs[2 p],
 * [2 p + 1] = record index of the first and the second of pair p in delivery order (at most cap_pairs pairs), waiting[] = the
 * records left waiting in window order (at most cap_waiting); info[0] = pairs, [1] = waiting, [2] = the newest record of a
 * name with more than 64 records of one class (then no pairs and no waiting records are given), ~0: none. */
enum { VS_BAM_COLLATED = 0, VS_BAM_BY_NAME = 1, VS_BAM_BY_NAME_KEEP = 2 };
int vs_bam_stream_open_mode(vs_ctx *ctx, const char *path, int mode, vs_bam_stream **out);
int vs_bam_stream_mate_info(const vs_bam_stream *s, uint64_t info[4]);
int vs_bam_mates_host(const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t hash_bits, uint32_t *pairs, uint64_t cap_pairs,
                      uint32_t *waiting, uint64_t cap_waiting, uint64_t info[3]);
int vs_bam_mates_text(vs_ctx *ctx, const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t hash_bits, uint32_t *pairs,
                      uint64_t cap_pairs, uint32_t *waiting, uint64_t cap_waiting, uint64_t info[3]);
/* Interleaved FASTQ (additions to ABI 11): ONE file or pipe in which each pair's two records follow each other (`samtools
 * fastq x.bam` to stdout, `seqtk mergepe`, `fastp --stdout`; what `bwa mem -p` reads), streamed as vs_fastq_stream_* streams
 * two files, in every form that stream reads.  Mates are found by NAME on the device, as `bwa mem -p` finds them.
 * A record is four lines: complete records = lines / 4, a final line without a newline counts at the end of the file, a
 * trailing group of fewer than four lines is ignored; '\r' and bytes >= 0x80 as in the two-file stream (names are compared
 * after that translation).  The name token of a record is its first line from its first byte up to (not including) the first
 * space (0x20), tab (0x09) or the line's end.  mates(a, b): take both tokens; if a's ends in "/1" AND b's in "/2" drop those
 * two bytes from both; true iff both are non-empty, of equal length and equal byte for byte ("a/2" then "a/1": no;
 * "a 1:N:0:x" then "a 2:N:0:x": yes; "a/1" then "a/1": yes; an empty token never matches).  Pairing is greedy from the front:
 *     i = 0;  while i < R:  if i + 1 < R and mates(i, i + 1): pair (i, i + 1), i += 2;  else: single i, i += 1
 * The result is by definition what vs_fastq_stream_* gives for the two files (first records of the pairs, second records of
 * the pairs).
 *   vs_fastq_il_open  : mode VS_IL_STRICT: the first single record fails the stream with VS_E_ARG -- the message names the
 *                       path, the file-wide 0-based record number and both header lines (the single's and its successor's,
 *                       or "end of file"); VS_IL_SINGLES: single records are dropped and counted; VS_IL_KEEP (an addition to
 *                       ABI 11, the other modes unchanged): classified as VS_IL_SINGLES, but the single records are KEPT -- when
 *                       the pairs of a window are out, its single records are handed out in file order as singles blocks
 *                       (vs_reads_pack_single above has the layout).  A record held back stays held; at the end of the file it
 *                       is a single and is handed out.  No mixed block is ever made
 *   vs_fastq_il_next  : as vs_fastq_stream_next; under VS_IL_KEEP *n_pairs is the number of SLOTS of the block and
 *                       vs_reads_unpaired tells its kind
 *   vs_fastq_il_info  : info[0] = pairs delivered, [1] = single records (dropped, or kept under VS_IL_KEEP), [2] = records decided, [3] = text bytes read
 *                       (inflated), [4] = file bytes read (compressed), [5] = flags as vs_fastq_stream_info (bit 2: gzip)
 *   vs_fastq_il_close : as vs_fastq_stream_close
 * Test aids, the match of ONE window of n text bytes as they are (no text-mode translation); eof: the file ends with the
 * window -- otherwise the last complete record is held back, unclassified, unless it is the second of a pair (its successor
 * has not been seen).  pairs[2 p], [2 p + 1] = record index of the first and the second of pair p (at most cap_pairs pairs);
 * info[0] = pairs, [1] = singles, [2] = records decided, [3] = the record held back (~0: none), [4] = the first single (~0:
 * none), [5] = complete records.  _host is the one-thread twin (vs_mates_core.h); _text runs the kernels and keeps `guard`
 * sentinel words on either side of the device pair list, VS_E_STATE if one changed or a word of the list stayed unwritten. */
enum { VS_IL_STRICT = 0, VS_IL_SINGLES = 1, VS_IL_KEEP = 2 };
typedef struct vs_fastq_il vs_fastq_il;
int vs_fastq_il_open(vs_ctx *ctx, const char *path, int mode, vs_fastq_il **out);
int vs_fastq_il_next(vs_ctx *ctx, vs_fastq_il *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs);
int vs_fastq_il_info(const vs_fastq_il *s, uint64_t info[6]);
void vs_fastq_il_close(vs_fastq_il *s);
int vs_fastq_mates_host(const uint8_t *text, uint64_t n, int eof, uint32_t *pairs, uint64_t cap_pairs, uint64_t info[6]);
int vs_fastq_mates_text(vs_ctx *ctx, const uint8_t *text, uint64_t n, int eof, uint32_t *pairs, uint64_t cap_pairs, uint32_t guard,
                        uint64_t info[6]);
/* An interleaved whole-BGZF file shared among ranks by member (additions to ABI 11 without a new number: nothing that exists
 * changes).  With m[j] = mates(j, j + 1) and p(0) = 0, p(j + 1) = m[j] ? !p(j) : 0, record j is the SECOND of a pair iff p(j) = 1.
 * A rank owns the records [a, b) = its share of the T complete records, every pair whose FIRST record it owns and every single
 * it owns.  A function of one bit is two bits, f(0) | f(1) << 1: const-0 = 0, flip = 1, identity = 2, const-1 = 3.  The
 * function of a share is the composition, in order, of flip (m true) or const-0 (m false) over m[a .. b - 1]; it takes p(a) to
 * p(b).
 *   vs_fastq_il_range_fn   : range = {file offset of the first member, offset one past the last, lines to skip in front} as
 *                            vs_fastq_stream_open_range takes it for one file.  *fn = the composition of m[0 .. n_rec - 2] of
 *                            the first n_rec records of the range (identity for n_rec < 2, nothing is read then): the range is
 *                            streamed window by window, the line ends scanned, the records matched and the windows' functions
 *                            composed on the device; nothing is packed or classified and no text returns to the host.  info[0]
 *                            = members inflated, [1] = file bytes read, [2] = windows, [3] = records seen.  A range with fewer
 *                            than n_rec records, or with a '\r' or a byte >= 0x80, is VS_E_STATE
 *   vs_il_shard_plan       : host only, pure.  fn[r] = the function of rank r's share (identity for an empty one; the last
 *                            rank's is not used); entry[r] = p of rank r's first record: entry[0] = 0, entry[r + 1] =
 *                            fn[r](entry[r])
 *   vs_fastq_il_open_range : the interleaved stream on a member range, mode VS_IL_STRICT or VS_IL_SINGLES (VS_IL_KEEP: VS_E_ARG).
 *                            The stream sees exactly n_owned + lookahead records behind the skipped lines.  entry = 1: the first
 *                            record is the second of the previous rank's last pair, neither handed out nor counted.  lookahead =
 *                            1: the last record is the next rank's first and the range does not end the file; classed second it
 *                            completes this rank's last pair and is packed here, otherwise it is discarded -- never a single,
 *                            never the start of a pair.  lookahead = 0: the range's end is the file's.  The record numbers of
 *                            the strict mode's message are file-wide: first_record + the number within the range.
 *                            vs_fastq_il_next / _info / _close serve the handle; pairs, singles and records count the rank's
 *                            own decisions, so their sums over the ranks are the whole file's.  The reader never reads at or
 *                            beyond range[1] */
int vs_fastq_il_range_fn(vs_ctx *ctx, const char *path, const uint64_t range[3], uint64_t n_rec, uint32_t *fn, uint64_t info[4]);
int vs_il_shard_plan(const uint32_t *fn, uint32_t world, uint32_t *entry);
int vs_fastq_il_open_range(vs_ctx *ctx, const char *path, int mode, const uint64_t range[3], uint64_t n_owned, int lookahead, uint32_t entry,
                           uint64_t first_record, vs_fastq_il **out);
/* ONE file of unpaired reads (additions to ABI 11 without a new number: nothing that exists changes): the unpaired survivors of
 * a trimmer, the merged reads of an overlapping library.  Streamed as vs_fastq_il_* streams one file, in every form that
 * stream reads (plain, FIFO, gzip through zlib, BGZF inflated on the device, plain gzip on the device with VS_GZIP_DEVICE=1),
 * without the matching: every complete record is one read.  Records, '\r', bytes >= 0x80, a final line without a newline and
 * a trailing group of fewer than four lines as there.  The blocks are singles blocks (vs_reads_pack_single above), built on
 * the device; no record text comes back to the host.
 *   vs_fastq_se_open  : opens the file and starts its reader
 *   vs_fastq_se_next  : the next block of up to max_reads reads (0 = 2^30), *n_reads = its reads = its slots; *out == NULL
 *                       at the end.  A sequence line of more than 2^24 - 1 bytes is VS_E_RANGE, the message names the path
 *                       and the file-wide 0-based record number
 *   vs_fastq_se_info  : info[0] = reads delivered, [1] = complete records seen, [2] = text bytes read (inflated), [3] = file
 *                       bytes read (compressed), [4] = flags as vs_fastq_il_info's info[5], [5] = 0
 *   vs_fastq_se_close : as vs_fastq_stream_close */
typedef struct vs_fastq_se vs_fastq_se;
int vs_fastq_se_open(vs_ctx *ctx, const char *path, vs_fastq_se **out);
int vs_fastq_se_next(vs_ctx *ctx, vs_fastq_se *s, uint64_t max_reads, vs_reads **out, uint64_t *n_reads);
int vs_fastq_se_info(const vs_fastq_se *s, uint64_t info[6]);
void vs_fastq_se_close(vs_fastq_se *s);
/* Two FASTQ files paired by READ NAME (additions to ABI 11): the two files of vs_fastq_stream_*, in every form that stream
 * reads, but a pair is a pair of mates by name, decided on the device.  Records, the name token and mates(a, b) as for the
 * interleaved FASTQ above; a = the header line of the file-1 record, b = that of the file-2 record.
 * KEY of a record: its token, without a trailing "/1" on a file-1 record and without a trailing "/2" on a file-2 record.  The
 * key only nominates: two records are a pair iff they are of different files, their keys are non-empty and equal byte for
 * byte, and mates(a, b) ("x/1" against "x": two singles).
 *   VS_PN_STRICT  : pair p is record p of either file and must be a pair of mates (mates(a_p, b_p), nothing else): the first
 *                   that is not fails the stream with VS_E_ARG -- the message names both paths, the file-wide 0-based pair
 *                   number and both header lines (at most 200 bytes each) -- and so does a complete record left over in the
 *                   longer file.
 *   VS_PN_SINGLES : the files are in the same order, either may lack records the other has.  An input is VALID when (V1)
 *                   within one file no non-empty key occurs twice and (V2) the file-1 records that have a mate, in file order,
 *                   have their mates in increasing file-2 order.  For a valid input the pairs are exactly the records whose
 *                   key is in both files (and mates), in file-1 order; every other complete record is a single of its file,
 *                   dropped and counted -- whatever the chunk size.  A V1 or V2 violation inside one pair of windows fails the
 *                   stream with VS_E_ARG ("name X occurs twice in FILE", "... are mates but lie behind ..."); one that spans
 *                   windows leaves its records among the singles.  A window beyond VS_PAIR_WINDOW bytes (environment; default
 *                   the largest window) none of whose records a round decided is VS_E_RANGE.  VS_PAIR_NAME_BITS (environment, tests)
 *                   keeps the low bits of the name hash only.
 *   VS_PN_KEEP    : (an addition to ABI 11, the other modes unchanged) the join, V1, V2, the refusals and what a round decides are
 *                   those of VS_PN_SINGLES, but the singles are KEPT.  A kept single of a round is a record the round decided
 *                   that is in none of its pairs; when the pairs of a round are out its kept singles are handed out as singles
 *                   blocks (vs_reads_pack_single above has the layout) of at most max_pairs slots, file 1's first in file
 *                   order, then file 2's in file order, and only then are the windows cut.  A record the round did not decide
 *                   is not handed out: it is in the next round's windows and is handed out exactly once, as half of a pair
 *                   or as a single.  For a valid input the kept reads of file f are exactly the complete records of file f
 *                   whose key is not in both files, in file order, whatever the chunk, window or block size.  No mixed block
 *                   is ever made.  As under VS_PN_SINGLES a V1 or V2 violation that spans windows leaves its records among
 *                   the singles: they are then counted as unpaired reads.
 *   vs_fastq_pn_next  : as vs_fastq_stream_next; under VS_PN_KEEP as vs_fastq_il_next under VS_IL_KEEP: *n_pairs is the number
 *                       of SLOTS of the block and vs_reads_unpaired tells its kind
 *   vs_fastq_pn_info  : info[0] = pairs delivered, [1] / [2] = singles of file 1 / file 2 (dropped, or kept under VS_PN_KEEP), [3] / [4] = records decided
 *                       of file 1 / file 2, [5] = rounds (pairs of windows joined), [6] = the largest window in bytes, [7] =
 *                       text bytes read, [8] = file bytes read, [9] = flags as vs_fastq_stream_info
 * Test aids, the join of ONE pair of windows (n0 / n1 text bytes as they are; eof0 / eof1: the file ends with its window; table:
 * slots of the open-address table, a power of two >= 2, 0: the stream's choice (>= 2 (R1 + R2)); name_bits: low bits of the
 * name hash kept, 0: all 64).  pairs[2 p], [2 p + 1] = file-1 and file-2 record of pair p (at most cap_pairs pairs); info[0] =
 * pairs, [1] / [2] = complete records of window 1 / 2, [3] / [4] = records of window 1 / 2 the round decides, [5] = a key
 * twice in one window: file << 32 | the smallest record involved (~0: none), [6] = the first pair whose file-2 record does not
 * lie behind that of the pair before (~0: none, also with [5] set), [7] = VS_PN_STRICT: the first pair that is no pair of mates (~0: none).  With
 * [5] or [6] set no pairs are given and nothing is decided.  _host is the one-thread twin (vs_pair_names_core.h), VS_E_STATE
 * when the table is full; _text runs the kernels and keeps `guard` sentinel words on either side of the device pair list
 * (room for min(R1, R2) pairs), VS_E_STATE if one changed, a word of the list stayed unwritten or one behind it was written.
 * vs_fastq_join_singles_host / _text: the same join (mode VS_PN_SINGLES or VS_PN_KEEP, the same result for both) and the kept
 * singles of the round as well: singles0[] / singles1[] = the decided records of window 1 / 2 that are in no pair, in order
 * (at most cap_singles0 / cap_singles1 of them), info[8] / [9] = how many there are; info[0..7] as above.  _host is the
 * one-thread twin; _text runs the compaction kernels with `guard` sentinel words on either side of both device lists,
 * VS_E_STATE if one changed or a word of a list stayed unwritten. */
enum { VS_PN_STRICT = 0, VS_PN_SINGLES = 1, VS_PN_KEEP = 2 };
typedef struct vs_fastq_pn vs_fastq_pn;
int vs_fastq_pn_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, int mode, vs_fastq_pn **out);
int vs_fastq_pn_next(vs_ctx *ctx, vs_fastq_pn *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs);
int vs_fastq_pn_info(const vs_fastq_pn *s, uint64_t info[10]);
void vs_fastq_pn_close(vs_fastq_pn *s);
int vs_fastq_join_host(const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                       uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint64_t info[8]);
int vs_fastq_join_text(vs_ctx *ctx, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                       uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t guard, uint64_t info[8]);
int vs_fastq_join_singles_host(const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                               uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t *singles0, uint64_t cap_singles0, uint32_t *singles1,
                               uint64_t cap_singles1, uint64_t info[10]);
int vs_fastq_join_singles_text(vs_ctx *ctx, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                               uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t *singles0, uint64_t cap_singles0, uint32_t *singles1,
                               uint64_t cap_singles1, uint32_t guard, uint64_t info[10]);
/* Member-sharded open of ONE collated BAM for one process per GPU (additions to ABI 10): no rank inflates the whole file and
 * nothing is inflated on a host.  Rank r of W takes the BGZF members [M r / W, M (r + 1) / W) of vs_bgzf_walk_file, its
 * "share": the inflated bytes [S_r, S_r + E_r).  A share cannot be entered at a guessed record start, so pass 1 follows the
 * chain from EVERY candidate start and the ranks exchange what each found (pe.BamStream.open_shard):
 *   vs_bam_share_summary : members [first, last) of the walk (offsets[n_members + 1], all of them: the whole members behind
 *                         the share that hold 64 inflated bytes, or the rest of the file, are read too and belong to no
 *                         count) inflated window by window on the device.  start = ~0: candidates c = 0 .. C - 1 with
 *                         C = min(seg, E) (positions relative to S_r); else the one candidate `start` (rank 0: vs_bam_header).
 *                         x[c] = the first position >= E the chain from c reaches, minus E; ~0 when it meets a block_size
 *                         < 32 first; ~0 - 1 when the end of the file cuts a size field or a record's fixed part.
 *                         cnt[c] = the participating records (first / second) that start on that chain inside the share.
 *                         seg = 0: VS_BAM_SEG, else 12288.  info[0] = C, [1] = E, [2] = members inflated, [3] = file bytes
 *                         read, [4] = windows.  A member the device rejects is VS_E_ARG in the stream's words
 *   vs_bam_share_summary_host / _text : test aids over inflated bytes share[0, n), n >= share_size + 64 unless the file ends
 *                         at n; windows of `chunk` new bytes (0: one window).  _host: the same text with one host thread,
 *                         _text: the kernels.  info[0] = C, [1] = windows
 *   vs_bam_shard_plan   : host only, a pure function of the gathered values.  head[6 r ..] = failed, whole BGZF, M, header
 *                         bytes H, E_r, C_r; xn + xn_off[r] = x_r[0 .. C_r) then cnt_r[0 .. C_r).  plan[5 r ..] = bytes in
 *                         front of rank r's first record (e_r - S_r), where its ownership ends relative to S_r (~0: the end
 *                         of the file), participating records in front of e_r, S_r, participating records in front of
 *                         e_{r+1}.  *reason = 0, or why every rank leaves the file to rank 0: 1 a rank failed, 2 the ranks
 *                         see different files, 3 not whole BGZF, 4 the header reaches beyond rank 0's share, 5 a record
 *                         longer than a segment across a share boundary or a share without bytes, 6 a block_size < 32 on
 *                         the chain, 7 the file ends inside a record, 8 the chain does not end at the end of the file, 9 an
 *                         odd number of participating records
 *   vs_bam_stream_open_range : the collated stream on range = {file offset of the share's first member, e_r - S_r, where
 *                         ownership ends relative to S_r (~0: none), 1 when the first participating record is the second
 *                         of the previous rank's last couple and is passed over, S_r}.  Couple c belongs to the rank whose
 *                         [e_r, e_{r+1}) holds the start of its first record; the second may start beyond, and the members
 *                         behind the range are inflated one by one for it and for nothing else.  next, info and close as
 *                         for the other modes; info counts the records that start in [e_r, e_{r+1}).  A message names a
 *                         record by its byte offset in the inflated file and says so. */
int vs_bam_share_summary(vs_ctx *ctx, const char *path, const uint64_t *offsets, uint64_t n_members, uint64_t first, uint64_t last, uint64_t start,
                         uint32_t seg, uint64_t *x, uint64_t *cnt, uint64_t cap, uint64_t info[5]);
int vs_bam_share_summary_host(const uint8_t *share, uint64_t n, uint64_t share_size, uint64_t start, uint32_t seg, uint64_t chunk, uint64_t *x,
                              uint64_t *cnt, uint64_t cap, uint64_t info[2]);
int vs_bam_share_summary_text(vs_ctx *ctx, const uint8_t *share, uint64_t n, uint64_t share_size, uint64_t start, uint32_t seg, uint64_t chunk,
                              uint64_t *x, uint64_t *cnt, uint64_t cap, uint64_t info[2]);
int vs_bam_shard_plan(uint32_t world, const uint64_t *head, const uint64_t *xn, const uint64_t *xn_off, uint64_t *plan, int *reason);
int vs_bam_stream_open_range(vs_ctx *ctx, const char *path, const uint64_t range[5], vs_bam_stream **out);
/* The header of a BAM at the front of a file (host: zlib on its leading BGZF members): *header_bytes = inflated bytes in
 * front of the first record.  VS_E_ARG with a message when the file is no BAM. */
int vs_bam_header(const char *path, uint64_t *header_bytes);

/* pe_info / st_info text (PE_Inference.py:194-205): "{id_i}:{id_j}:{count}\n" for all i, j in
 * row-major order, zeros included.  ids: the n node names concatenated, id_off[n+1]; mat: HOST
 * n*n int64.  Formatted on all host cores, one write(). */
int vs_write_matrix_text(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off,
                         uint32_t n, const int64_t *mat);

/* Sparse pe_info / st_info (additions to ABI 10): the dense file above with every line removed whose count is 0, the other
 * lines in their order (row-major in the caller's node order, ids written as the dense writer writes them).  A matrix of
 * zeros gives a file of 0 bytes; no empty line is ever written (the reference stops reading at one).  The reference reads
 * such a file to the same dict as the dense one: process_pe_info (utils/VStrains_IO.py:598-623) sets every key to 0 before
 * it adds the lines.
 *   vs_write_info_sparse      : formatted ON THE DEVICE from the counters where they lie -- no permuted copy, no download of
 *                               a matrix, no sort.  d_counts: DEVICE n*n uint32 cells in the index's internal numbering (may
 *                               be NULL); d_wide: DEVICE n*n int64 totals (vs_counts_fold; may be NULL; one of the two must
 *                               be given); a cell's total is the sum of both.  d_tile_map: DEVICE T*T bytes, T = ceil(n / 64),
 *                               THIS matrix's half of the dirty-tile map of vs_pe_count_tracked, or NULL: a cell of d_counts
 *                               in an unmarked tile is taken as 0 without being read (d_wide is always read).  rank: HOST,
 *                               rank[i] = internal number of the caller's node i (NULL = the same numbering).  The value of
 *                               the caller's cell (i, j), with a = rank[i], b = rank[j]:
 *                                 upper == 0 (node_mat)  M[a][b]
 *                                 upper == 1 (short_mat) 0 for i > j, S[a][a] for i == j, S[a][b] + S[b][a] otherwise
 *                               A negative total is VS_E_ARG.  Two passes (k_info_row_sizes: lines and bytes per row;
 *                               k_info_format: the text of a block of whole rows of at most 256 MB, VS_TEXT_BLOCK as in
 *                               vs_write_matrix_text), two device / pinned buffer pairs: block k + 1 is formatted while
 *                               block k is written.  info (may be NULL): [0] lines, [1] bytes, [2] blocks written,
 *                               [3] counter cells read (a cell skipped through the tile map is not).
 *   vs_write_info_sparse_host : the host twin.  The same arguments as HOST pointers, ctx may be NULL, one thread; it runs the
 *                               text the kernels run (csrc/vs_info_core.h) and writes the same bytes. */
int vs_write_info_sparse(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n,
                         const uint32_t *d_counts, const int64_t *d_wide, const uint8_t *d_tile_map, const uint32_t *rank,
                         int upper, uint64_t info[4]);
int vs_write_info_sparse_host(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n,
                              const uint32_t *counts, const int64_t *wide, const uint8_t *tile_map, const uint32_t *rank,
                              int upper, uint64_t info[4]);

/* pe_info / st_info as BGZF, deflated on the device (additions to ABI 10): `gzip -dc`, `zcat` and Python's gzip give back
 * the text, bgzip-aware tools can seek in it.  Arguments as vs_write_info_sparse.  dense == 0: the sparse text above;
 * dense == 1: EVERY line of the reference's file in row-major order, zeros included (for upper == 1 the lines below the
 * diagonal too, with the count 0) -- the file utils/VStrains_PE_Inference.py writes, byte for byte, once inflated.  Per block
 * of text (whole rows, at most 256 MB, VS_TEXT_BLOCK): k_info_format writes the text into a device buffer, k_deflate makes
 * the block's members (members never span blocks: a block's last member is short), they are packed back to back on the device
 * from the scan of their sizes, and ONLY those bytes are copied to a pinned buffer and written; two buffer pairs alternate.
 * No text and no matrix leaves the device.  The 28-byte EOF member ends the file: a matrix of zeros, sparse, is that member
 * alone.  Errors as vs_write_info_sparse; a member that ends with a status other than 0 is VS_E_STATE and names the member.
 * info (may be NULL): [0] lines, [1] text bytes, [2] blocks, [3] counter cells read, [4] members without the EOF member,
 * [5] file bytes.
 *   vs_write_info_bgzf_host : the host twin.  The same arguments as HOST pointers, ctx may be NULL, one thread, the same bytes. */
int vs_write_info_bgzf(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n,
                       const uint32_t *d_counts, const int64_t *d_wide, const uint8_t *d_tile_map, const uint32_t *rank,
                       int upper, int dense, uint64_t info[6]);
int vs_write_info_bgzf_host(vs_ctx *ctx, const char *path, const uint8_t *ids, const uint64_t *id_off, uint32_t n,
                            const uint32_t *counts, const int64_t *wide, const uint8_t *tile_map, const uint32_t *rank,
                            int upper, int dense, uint64_t info[6]);

/* (addition to ABI 10) A pe_info / st_info file, dense or sparse, parsed on the host threads into cells against a name list:
 * the lines up to the first empty one; each line minus its LAST CHARACTER (the newline, or a real character on a final line
 * without one) split at ':', the first three fields taken (IO.py:603-612); a line naming an id that is not among the n names
 * (concatenated in `names`, name_off[n + 1]) is skipped.  Fewer than three fields, or a count that is not an optionally
 * signed decimal integer that fits int64, is VS_E_ARG (vs_last_error(NULL) quotes the line).  rows / cols / vals receive
 * up to cap cells in file order; with cap == 0 nothing is parsed and info[0] is the number of lines, an upper bound on the
 * cells.  info[0] = cells, [1] = flags: bit 0 the file holds a '\r', bit 1 a byte >= 0x80 -- such a file is NOT parsed here
 * (universal newlines and the text decoding belong to Python: the caller keeps its own loop), [2] = lines read,
 * [3] = lines skipped for an unknown id.  A file that starts with the gzip magic 1f 8b (what vs_write_info_bgzf writes, or
 * any gzip) is first inflated on the host with zlib, all members of it, and then read exactly as the plain file is; a cut-off
 * or corrupt stream is VS_E_ARG with zlib's words. */
int vs_info_parse(const char *path, const uint8_t *names, const uint64_t *name_off, uint32_t n, uint32_t *rows, uint32_t *cols,
                  int64_t *vals, uint64_t cap, uint64_t info[4]);
/* (addition to ABI 10) The host twin of the device reader below (vs_links_from_info): text[0, size) held by the caller, read
 * by the rules of vs_info_parse through the code the kernels run (csrc/vs_info_read_core.h), one thread, in windows of
 * window_bytes (0 = 256 MB, at least 16) whose buffer always begins at a line start.  rows / cols / vals receive up to cap cells
 * in text order (more is VS_E_RANGE).  info[0] = outcome: 0 read, 1 the text holds a '\r' or a byte >= 0x80 (Python's to read),
 * 2 a malformed line, 3 a line does not fit a window (the file is vs_info_parse's); [1] lines, [2] lines skipped for an unknown
 * id, [3] cells, [4] text offset of the first malformed line, [5] windows, [6] flags as vs_info_parse's info[1], [7] text bytes. */
int vs_info_read_host(const uint8_t *text, uint64_t size, const uint8_t *names, const uint64_t *name_off, uint32_t n,
                      uint64_t window_bytes, uint32_t *rows, uint32_t *cols, int64_t *vals, uint64_t cap, uint64_t info[8]);

/* Synthetic pairs generated on the device from a seed (bench workload; the CPU twin is
 * oracle/pe_oracle.c:peo_synth_pairs).  genomes: concatenated ACGT ASCII (host), goff
 * [n_strains+1]; cum[s]: inclusive upper bound of strain s in a uniform u32 draw (last =
 * 0xFFFFFFFF).  sub_thresh / n_thresh: u32 thresholds (rate * 2^32) for per-base
 * substitutions and for pairs that get one 'N'.  Pairs first_pair .. first_pair+n_pairs-1 of
 * the stream are produced, so ranks can take disjoint slices of one stream. */
int vs_synth_pairs(vs_ctx *ctx, const uint8_t *genomes, const uint64_t *goff,
                   const uint32_t *cum, uint32_t n_strains, uint64_t seed, uint64_t first_pair,
                   uint64_t n_pairs, uint32_t read_len, uint32_t sub_thresh, uint32_t n_thresh,
                   vs_reads **out);

/* ---- K2-K4: PE-link counting ----------------------------------------------------------------
 * Replaces PE_Inference.py:155-188 (pair filters, single_end_read_mapping on both ends,
 * short_mat / node_mat updates) for all pairs of `reads`.
 * d_node_mat, d_short_mat: DEVICE pointers to N*N row-major uint32 counters, d_stats: DEVICE
 * pointer to 3 uint64 {n_reads, short_reads, used_reads}.  Counts are ADDED (atomically), so
 * several blocks / ranks can accumulate and the caller all-reduces (RCCL) as it likes.
 * A cell grows by at most 2 per pair (short_mat[i][i] is incremented once per end, :174-184), so
 * uint32 is exact while 2 * (pairs counted into one buffer, over all ranks that will be summed
 * into it) < 2^32; vs_counts_fold moves a buffer into int64 totals before that. */
int vs_pe_count(vs_ctx *ctx, const vs_reads *reads, uint32_t *d_node_mat, uint32_t *d_short_mat,
                uint64_t *d_stats);

/* The same with a record of WHERE the counts went: d_tile_map holds one byte per 64 x 64 tile of node_mat followed by one
 * per tile of short_mat (2 * T * T bytes, T = ceil(N / 64), DEVICE memory, zero before the first call); the tiles the
 * block adds to are set to 1.  A caller that wants empty counters for the next block then calls vs_counts_zero_tracked
 * -- zero every marked tile, clear the map -- instead of clearing 2 * N * N cells: the counters of a 50 k-node graph are
 * 23.7 GB and a block touches a few per cent of them.  (The reference allocates its matrices once, PE_Inference.py:
 * 139-140; per-block zeroing exists only where a caller counts blocks separately, as bench.py's steps do.)  Ranks that
 * sum their counters must OR their maps too before they zero (a maximum over the bytes). */
int vs_pe_count_tracked(vs_ctx *ctx, const vs_reads *reads, uint32_t *d_node_mat, uint32_t *d_short_mat,
                        uint64_t *d_stats, uint8_t *d_tile_map);
int vs_counts_zero_tracked(vs_ctx *ctx, uint32_t *d_node_mat, uint32_t *d_short_mat, uint32_t n, uint8_t *d_tile_map);

/* d_wide[i] += d_counts[i] (read as uint32); d_counts[i] = 0, for i < n.  DEVICE pointers.  The
 * reference's matrices are numpy.zeros(..., dtype=int) = int64 (PE_Inference.py:139-140): a caller
 * that counts more pairs than a uint32 cell can hold folds into int64 totals in between. */
int vs_counts_fold(vs_ctx *ctx, uint32_t *d_counts, int64_t *d_wide, uint64_t n);

/* (ABI 8) d_occ[j] = 1 where the j-th stretch of 64 consecutive cells (cell_bytes = 4: uint32 counters, 8: int64 totals)
 * holds a non-zero cell, else 0, for j < n_stretches.  DEVICE pointers.  No counterpart in the reference (single
 * process): the ranks of a multi-GPU run exchange only the occupied stretches of their counters (the non-zero cells of
 * node_mat / short_mat, PE_Inference.py:174-188, lie in a band), and this is the one pass over the buffer that finds them. */
int vs_counts_occupied(vs_ctx *ctx, const void *d_cells, uint32_t cell_bytes, uint64_t n_stretches, uint8_t *d_occ);

/* ---- C1: sum of the counters over ranks (RCCL over xGMI) ---------------------------------------
 * No counterpart in the reference (single process); read pairs are independent and the counters
 * add (PE_Inference.py:174-188), so ranks count disjoint read blocks and sum.  One process per
 * GPU.  The RCCL library is resolved at the first call (the copy already loaded into the process,
 * else librccl.so.1); without it the calls fail with VS_E_HIP.
 *   vs_comm_unique_id : rank 0 makes the 128-byte id and hands it to the other ranks out of band
 *   vs_comm_init_rank : collective over the n_ranks processes; *comm receives an ncclComm_t
 *   vs_pe_allreduce   : in-place ncclAllReduce(ncclSum) of node_mat[n*n], short_mat[n*n] (uint32,
 *                       or int64 totals when `wide` != 0) and of the 3 uint64 stats, enqueued on the
 *                       ctx stream.  `comm` is an ncclComm_t made by vs_comm_init_rank or by the
 *                       caller's own RCCL calls in this process.  DEVICE pointers. */
int vs_comm_unique_id(vs_ctx *ctx, uint8_t id[128]);
int vs_comm_init_rank(vs_ctx *ctx, int n_ranks, const uint8_t id[128], int rank, void **comm);
int vs_comm_destroy(vs_ctx *ctx, void *comm);
int vs_pe_allreduce(vs_ctx *ctx, void *comm, void *d_node_mat, void *d_short_mat, uint64_t *d_stats,
                    uint32_t n, int wide);

/* Per-end result of single_end_read_mapping (PE_Inference.py:16-48) for testing: for each end
 * e, counts[e] = number of accepted nodes (0 for ends of pairs the filters drop), and up to
 * `cap` of them, ascending, in lists[e*cap ...].  Host pointers. */
int vs_pe_map_ends(vs_ctx *ctx, const vs_reads *reads, uint32_t cap, uint32_t *lists,
                   uint32_t *counts);

/* Timing of the most recent vs_pe_count on this ctx, measured with HIP events on the ctx
 * stream: ms[0] = mapping kernel (k_pe_tiles), ms[1] = overflow (slow-path) kernel, ms[2] =
 * pairs sent to the slow path, ms[3] = locus ordering of the pairs in front of the mapping
 * kernel (k_pe_locus + scan + k_pe_permute), ms[4] = counter kernels (k_pe_accumulate, or the row
 * owners k_list_owners .. k_rows_sum on graphs beyond 46 340 nodes).
 * Synchronises the stream. */
int vs_pe_last_timing(vs_ctx *ctx, double ms[5]);
/* Name of the mapping-kernel instantiation the most recent vs_pe_count launched, as a profiler
 * prints it (e.g. "k_pe_tiles<true, 10u, 5u>"); "" before the first call. */
const char *vs_pe_last_kernel(const vs_ctx *ctx);
/* Which of the optional kernels the most recent vs_pe_count launched (a run's choice by graph size and read shape): */
enum {
    VS_RAN_LOCUS_LDS_SORT = 1,    /* locus order by per-workgroup LDS histograms (k_locus_count / k_locus_scatter) */
    VS_RAN_LOCUS_GLOBAL_SORT = 2, /* ... by global atomics (k_pe_locus / k_pe_permute): graphs beyond 147 k nodes */
    VS_RAN_LOCUS_STAGED = 4,      /* the keys of the LDS sort came from read words staged through LDS (k_locus_count_staged) */
    VS_RAN_PE_MID = 8,            /* overflow pairs through the wavefront-per-pair kernel first (k_pe_mid) */
    VS_RAN_ROW_OWNERS = 16        /* counters summed by row owners (k_list_owners / k_rows_count / k_rows_fill / k_rows_sum): graphs beyond 46 340 nodes */
};
uint32_t vs_pe_last_launched(const vs_ctx *ctx);

/* Testing aids (additions to ABI 10, like vs_index_export): the counter stage of a PE count alone, and the locus order of
 * the most recent count, observed.
 *   vs_pe_count_lists : the kernels between the mapping kernel and the matrices (k_mark_tiles, k_pe_accumulate, or the row
 *       owners k_list_owners .. k_rows_sum) on a block of per-end node lists the caller made up.  No index, no reads: the
 *       launch plan is the one vs_pe_count would make for n_nodes nodes and 2 * n_pairs ends of 150 bases at k = 55, with
 *       the context's switches; the lists are written into the hand-off layout that plan names and the host code a real
 *       count runs behind its mapping kernel is launched.  HOST pointers: lists = 2 * n_pairs rows of 20 words (left end,
 *       right end of pair 0, of pair 1, ...), counts[2 * n_pairs] = nodes per row, 0 .. 20, handed over in the order
 *       given.  DEVICE pointers: the matrices (n_nodes * n_nodes uint32 each, ADDED to) and d_tile_map (may be NULL; as
 *       vs_pe_count_tracked).  VS_E_RANGE, nothing launched: a count above 20, a node >= n_nodes, a node twice in one
 *       list, a tile of the plan (vs_pe_lists_ept ends) whose lists need more than ends * 4 quads of four nodes.
 *       vs_pe_last_launched says VS_RAN_ROW_OWNERS as after a count.
 *   vs_pe_lists_ept   : the read ends per tile of that plan on this context now (64 unless an experiment context says
 *       otherwise): a caller keeps a tile's lists inside its region by closing it early with empty pairs.
 *   vs_pe_last_order  : keys[i] = locus key of pair i, perm[j] = the pair the mapping kernel took j-th, of the most recent
 *       vs_pe_count / vs_pe_map_ends, copied to HOST memory (at most cap of each; either may be NULL); changes nothing.
 *       info[0] = pairs of that call, info[1] = the sort that ran: 0 none (input order; keys and perm are not written),
 *       VS_RAN_LOCUS_LDS_SORT or VS_RAN_LOCUS_GLOBAL_SORT. */
int vs_pe_count_lists(vs_ctx *ctx, uint32_t n_nodes, uint64_t n_pairs, const uint32_t *lists, const uint32_t *counts,
                      uint32_t *d_node_mat, uint32_t *d_short_mat, uint8_t *d_tile_map);
uint32_t vs_pe_lists_ept(vs_ctx *ctx);
int vs_pe_last_order(vs_ctx *ctx, uint32_t *keys, uint32_t *perm, uint64_t cap, uint64_t info[2]);
/* Testing aid (addition to ABI 11 without a new number, like vs_pe_last_order): the hand-off between the mapping kernel and
 * the counter kernels exactly as k_pe_tiles left it in the context's scratch at the most recent vs_pe_count /
 * vs_pe_count_tracked, copied to HOST memory.  Launches nothing and changes nothing; synchronises the stream.
 *   info[0] = 1 if that call made a hand-off, 0 if not (vs_pe_map_ends, vs_pe_count_lists, an empty block, no call yet):
 *             every other word is 0 then and nothing is copied
 *   info[1] = pairs of the call, info[2] = read ends per tile, info[3] = end slots (tiles * ends per tile)
 *   info[4] = layout: 0 packed (counts = n | quad offset inside the tile's region << 8), 1 rows (counts = n)
 *   info[5], info[6] = slots of the tile's (end, node) table and list trim of the k_pe_tiles instantiation that ran: a
 *             tile's packed lists take at most (ends per tile * 16 - trim) / 4 quads
 *   info[7] = pairs on the first overflow list (what k_pe_tiles sent on, not what k_pe_mid then left for k_pe_slow)
 *   info[8] = words of the list buffer in that layout
 *   lists[info[8]], counts[info[3]], overflow[info[7]]: at most cap_* words of each are written; any may be NULL.  The end
 *   slots of the last tile past 2 * pairs are not the mapping kernel's: the host zeroes their counts before the counter
 *   kernels run.  In the row layout only the quads that hold nodes are written by the kernel. */
int vs_pe_last_handoff(vs_ctx *ctx, uint32_t *lists, uint64_t cap_words, uint32_t *counts, uint64_t cap_ends, uint32_t *overflow,
                       uint64_t cap_overflow, uint64_t info[9]);
/* Testing aid (addition to ABI 11 without a new number, like vs_pe_last_handoff): where the overflow pairs of the most recent
 * vs_pe_count / vs_pe_count_tracked / vs_pe_map_ends went, copied to HOST memory.  Launches nothing and changes nothing;
 * synchronises the stream.
 *   info[0] = 1 if that call launched the overflow kernels, 0 if not (an empty block, vs_pe_count_lists, a call that failed
 *             before its launch, no call yet): every other word is 0 then and nothing is copied
 *   info[1] = pairs on the first overflow list (what k_pe_tiles gave up)
 *   info[2] = pairs k_pe_mid passed on to k_pe_slow (beyond its 64 probes, 256 touched or 64 accepted nodes per end)
 *   info[3] = 1 if k_pe_mid was skipped (VS_NO_MID on an experiment context: k_pe_slow took the first list; info[2] = 0)
 *   second[info[2]]: those pairs, in the order k_pe_mid's atomics took; at most cap are written; may be NULL. */
int vs_pe_last_overflow(vs_ctx *ctx, uint32_t *second, uint64_t cap, uint64_t info[4]);

/* ---- segment depth from the reads (additions to ABI 11 without a new number: nothing that exists changes) ------------
 * No counterpart in the reference, which takes a segment's depth from the assembler's DP:f or KC:i / LN:i tag
 * (utils/VStrains_IO.py:49-77).  SPAdes' KC:i is the number of (k+1)-mer occurrences of the segment in the reads, and the
 * reference's PE table (PE_Inference.py:117-135) is the table of the nodes' (k+1)-mers, so with K = k + 1:
 *   KC[n] = the number of triples (read end e, read offset i, table entry of node n) for which end_e[i : i + K] is a key
 *           of that table holding the entry
 * -- the sum, over all read ends, of the `v` single_end_read_mapping computes per node (PE_Inference.py:29) BEFORE its
 * acceptance test.  Deliberately: a palindromic window counts twice (the table holds it twice); a (k+1)-mer at several
 * node positions counts at each; a window over a byte outside ACGT counts nowhere; an end shorter than K, of length 0 or
 * absent (a singles block) counts nothing; EVERY end of the block counts, also the ends of pairs the PE filter drops
 * ('N' in the mate, short mate): depth is a property of k-mers, not of pairs.  tests/node_depth_model.py states it.
 *   vs_node_depth     : one block through k_node_depth on the context's CURRENT index (a later vs_index_build replaces it,
 *                       as above); d_kc: DEVICE pointer to n_nodes uint64 totals in the numbering vs_index_build was
 *                       given, ADDED to (atomically), so blocks accumulate.  Enqueued on the ctx stream.  The lists, the
 *                       locus sort and the PE counters are not involved, and vs_pe_last_* are left as they were.
 *   vs_ctx_keep_masks : on != 0: every read block built on this context from now on keeps its validity mask.  The PE count
 *                       never maps an end with an 'N', so a block whose only bytes outside ACGT are 'N's gives its mask
 *                       back (and the mapped ingest packs such a block on the host without one); the depth pass counts
 *                       those ends and needs their 'N's.  Call it before the blocks of a depth pass are built: in a block
 *                       without a mask an 'N' is read as the base it was packed as.  A PE count of a block that kept its
 *                       mask gives the same counters, by the generic mapping kernel where the block has no position lists.
 *   vs_depth_plan     : host only, a pure function (csrc/vs_depth_plan.h): the launch vs_node_depth makes for a graph of
 *                       n_nodes nodes at ksize and a block of n_ends ends of at most max_len bases on a device of n_cu
 *                       compute units.  plan[0] = route: 0 nothing launched (no end holds a window), 1 dense uint32
 *                       counters per node in LDS, 2 global (graphs of more than plan[6] nodes: credits combined per
 *                       wavefront, then added to the totals); [1] = workgroups; [2] = ends per workgroup; [3] = the most
 *                       ends per workgroup for which ends * (max_len - K + 1) < 2^32, the bound under which no LDS counter
 *                       wraps ([2] <= [3]); [4] = LDS counters; [5] = LDS bytes per workgroup; [6] = the node limit of
 *                       route 1; [7] = threads per workgroup.  VS_E_RANGE: more than 2^25 - 2 nodes, 2^32 ends. */
int vs_node_depth(vs_ctx *ctx, const vs_reads *reads, uint64_t *d_kc);
int vs_ctx_keep_masks(vs_ctx *ctx, int on);
int vs_depth_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t plan[8]);

/* ---- contigs threaded through the graph (additions to ABI 11 without a new number: nothing that exists changes) --------
 * No counterpart in the reference, which takes the contigs' walks from SPAdes' contigs.paths.  A contig that spells a walk
 * of the graph is a chain of maximal exact matches against consecutive segments, each overlapping the next by k bases;
 * tests/contig_thread_model.py states the rule window by window, csrc/vs_contig_chain.h at the level of matches.
 * A match record is five uint32: contig, first base in the contig, segment | strand << 31 (strand 1: on the segment's
 * reverse complement), first base in that strand's text, length in bases (>= k + 1).  A token is four: contig,
 * segment | strand << 31, windows of the contig it was chosen for, 1 if it opens a part.
 *   vs_contig_mems      : reads != NULL: one block through k_contig_mems on the context's CURRENT index -- every maximal
 *                         exact match of k + 1 bases or more between an end and a strand of a segment, once, in no order.
 *                         `contig` is the read of a singles block (vs_reads_pack_single), else the end.  Build the block
 *                         after vs_ctx_keep_masks(ctx, 1): a byte outside ACGT bounds a match only where its mask was
 *                         kept.  The records stay on the device, in a buffer of the context that grows to what a pass
 *                         found (the pass then runs a second time; nothing is cut off).  Synchronises the ctx stream.
 *                         reads == NULL: nothing runs, the last pass's records are meant.  Either way *n = their number,
 *                         and they are copied to HOST out[cap records] when cap >= *n (out may be NULL: ask, then fetch).
 *                         VS_E_RANGE: 2^32 ends, or 2^32 probes in one block (about 2^32 * (k + 2 - seed length) bases).
 *   vs_contig_mems_last : info[0] = records of the last pass, [1] launches of k_contig_mems it took (2: the buffer grew),
 *                         [2] probes, [3] the buffer's capacity in records when the pass began.
 *   vs_contig_chain     : host only, a pure function (csrc/vs_contig_chain.h): n_mems records in any order -> tokens[n_mems
 *                         x 4] (at most one per record) in contig order, *n_tokens, and ambiguous[n_contigs] = windows of
 *                         each contig with more than one hit.  seg_len[n_segs]: the segments' lengths in bases, in the
 *                         numbering of the records.  VS_E_ARG: a record names a contig or segment out of range, is
 *                         shorter than k + 1, or leaves its segment. */
int vs_contig_mems(vs_ctx *ctx, const vs_reads *reads, uint32_t *out, uint64_t cap, uint64_t *n);
int vs_contig_mems_last(vs_ctx *ctx, uint64_t info[4]);
int vs_contig_chain(const uint32_t *mems, uint64_t n_mems, const uint32_t *seg_len, uint32_t n_segs, uint32_t ksize, uint32_t n_contigs,
                    uint32_t *tokens, uint64_t *n_tokens, uint64_t *ambiguous);

/* ---- per-position depth of every segment from the reads (additions to ABI 11 without a new number: nothing that exists
 * changes) ------------------------------------------------------------------------------------------------------------
 * No counterpart in the reference.  With K = k + 1, for segment n and forward offset p in [0, len_n - K]:
 *   cov[n][p] = the number of triples (read end e, read offset i, table entry (n, p)) for which end_e[i : i + K] is a key
 *               of the reference's table (PE_Inference.py:117-135) holding that entry
 * -- the triples KC[n] of vs_node_depth counts, kept apart by their entry's offset, so sum_p cov[n][p] == KC[n] exactly
 * and every rule of that pass holds (palindromes twice, at ONE position; repeats at each; bytes outside ACGT nowhere; short,
 * empty and absent ends nothing; every end of every block).  The value belongs to the window that STARTS at p: k-mer
 * coverage, not base coverage.  tests/depth_profile_model.py states it; csrc/vs_cover_plan.h has the slots and the fold rule.
 * Slots: segment n of the index's own numbering owns len_n - K + 2 of them when len_n >= K, else none: one per window and
 * one sentinel behind them, which takes the -1 of a match flush with the segment's end and is 0 after every fold.
 *   vs_cover_layout : d_first: DEVICE pointer to n_nodes + 1 words, written: the first slot of every segment of the
 *                     context's CURRENT index, in the numbering vs_index_build was given, and the slot total S behind them;
 *                     *n_slots = S (host).  Synchronises the ctx stream.  VS_E_RANGE: S >= 2^32 (*n_slots is still set).
 *   vs_node_cover   : one block through k_node_cover on the context's current index: every maximal exact match of K bases
 *                     or more between an end and a strand of a segment adds +1 to the slot of its first window and -1 to
 *                     the slot behind its last, on d_diff (DEVICE, S uint32, zero before the first block, wrap-around
 *                     adds, atomically).  d_first: what vs_cover_layout wrote for THIS index.  Enqueued on the ctx stream.
 *                     Blocks must have been built after vs_ctx_keep_masks(ctx, 1).  VS_E_RANGE: 2^32 ends, or a block
 *                     whose ends could put 2^32 on one window (n_ends * 2 * (max_len - K + 1) >= 2^32).
 *   vs_cover_fold   : d_cov[i] += (excl[i] + d_diff[i]) mod 2^32 for the exclusive scan excl of d_diff over all S slots
 *                     (scratch of the context: 4 bytes per slot), and d_diff[i] = 0.  d_cov: DEVICE, S uint64 totals.
 *                     Enqueued on the ctx stream.  Right as long as no window gathered 2^32 since the last fold:
 *   vs_cover_plan   : host only, a pure function (csrc/vs_cover_plan.h): for a graph of n_nodes nodes at ksize, a block of
 *                     n_ends ends of at most max_len bases, a device of n_cu compute units, `pending` = plan[5] of the
 *                     block before (0 after a fold or at the start) and `bound` (0: 2^32; at most 2^32):
 *                     plan[0] = 1 if k_node_cover is launched (0: no end holds a window); [1] = workgroups; [2] = ends per
 *                     workgroup; [3] = the block's weight n_ends * 2 * (max_len - K + 1), the most it can add to one slot;
 *                     [4] = 1 if vs_cover_fold is due BEFORE this block (pending > 0 and pending + weight >= bound);
 *                     [5] = the weight pending once the block is counted; [6] = LDS bytes per workgroup; [7] = threads per
 *                     workgroup.  VS_E_RANGE: more than 2^25 - 2 nodes, 2^32 ends, a weight of 2^32 or more, bound or
 *                     pending beyond 2^32. */
int vs_cover_layout(vs_ctx *ctx, uint32_t *d_first, uint64_t *n_slots);
int vs_node_cover(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t *d_diff);
int vs_cover_fold(vs_ctx *ctx, uint32_t *d_diff, uint64_t *d_cov, uint64_t n_slots);
int vs_cover_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound,
                  uint64_t plan[8]);

/* ---- base pileup of every segment from the reads (additions to ABI 11 without a new number: nothing that exists changes) --
 * No counterpart in the reference.  With K = k + 1 and a mismatch budget M: a read end e, a strand t of a segment n with
 * len_n >= K (its forward text or the reverse complement) and a diagonal d = strand offset - read offset make a candidate
 * alignment whose OVERLAP is the read offsets x with 0 <= x < len_e and 0 <= x + d < len_n.  A position AGREES when the read
 * byte is one of ACGT and equals the strand's base.  The alignment is ANCHORED when its overlap holds K agreeing positions in
 * a row (a maximal exact match as vs_node_cover finds them) and CREDITED when at most M positions of the whole overlap do
 * not agree (a byte outside ACGT does not agree); it counts once, however many exact matches lie on its diagonal; a rejected
 * one deposits nothing and is tallied.  For every overlap position of a credited alignment, p its forward offset on the
 * segment: depth[n][p] += 1, and where it does not agree alt[n][p][c] += 1, c the read's base as it reads on the forward
 * strand (0..3 = ACGT, complemented for the reverse-complement strand; 4 = a byte outside ACGT).  The rules of the depth
 * pass hold (a palindromic overlap is two alignments; a read fitting twice counts at each; short, empty and absent ends
 * nothing; every end of every block).  Substitutions only: an indel ends the diagonal.  tests/pileup_model.py states it;
 * csrc/vs_pileup_plan.h has the slots and the fold rule, csrc/vs_pileup_core.h the walk along the diagonal.
 * Slots: segment n of the index's own numbering owns len_n + 1 of them when len_n >= K, else none: one per position and one
 * sentinel behind them, which takes the -1 of an overlap flush with the segment's end and is 0 after every fold.
 *   vs_pileup_layout    : d_first: DEVICE pointer to n_nodes + 1 words, written: the first slot of every segment of the
 *                         context's CURRENT index, in the numbering vs_index_build was given, and the slot total S behind
 *                         them; *n_slots = S (host).  Synchronises the ctx stream.  VS_E_RANGE: S >= 2^32 (*n_slots is set).
 *   vs_node_pileup      : one block through k_node_pileup on the context's current index.  Every credited alignment adds +1
 *                         to the slot of its overlap's first forward position and -1 to the slot behind its last, on d_diff
 *                         (DEVICE, S uint32, zero before the first block, wrap-around adds, atomically; folded into uint64
 *                         totals by vs_cover_fold, which is generic over a slot array), and 1 to d_alt[slot * 5 + c]
 *                         (DEVICE, S x 5 uint64, zero before the first block) per non-agreeing position.  d_tally: DEVICE,
 *                         2 uint64, added to: alignments credited, alignments rejected (anchored, more than max_mismatch
 *                         non-agreeing positions).  d_first: what vs_pileup_layout wrote for THIS index.  Enqueued on the ctx
 *                         stream.  Blocks must have been built after vs_ctx_keep_masks(ctx, 1).  VS_E_RANGE: 2^32 ends, or
 *                         a block whose ends could put 2^32 on one position (n_ends * 2 * max_len >= 2^32).
 *   vs_pileup_plan      : host only, a pure function (csrc/vs_pileup_plan.h), with the arguments and the fields of
 *                         vs_cover_plan: plan[0] = 1 if k_node_pileup is launched (0: no end holds K bases); [1] =
 *                         workgroups; [2] = ends per workgroup; [3] = the block's weight n_ends * 2 * max_len, the most it
 *                         can add to one slot; [4] = 1 if vs_cover_fold is due BEFORE this block (pending > 0 and pending +
 *                         weight >= bound); [5] = the weight pending once the block is counted; [6] = LDS bytes per
 *                         workgroup; [7] = threads per workgroup.  VS_E_RANGE: more than 2^25 - 2 nodes, 2^32 ends, a weight
 *                         of 2^32 or more, bound or pending beyond 2^32.
 *   vs_pileup_scan_host : host only, no device: the walk of csrc/vs_pileup_core.h, the code the kernel runs, on HOST buffers.
 *                         read_words / strand_words: packed texts (2 bits a base, 16 a word, first base lowest; A C G T =
 *                         0 1 2 3) of rlen / tlen bases, each with 3 zero words behind its last word; read_mask: NULL, or
 *                         the same layout with 0b11 where the read's byte is outside ACGT.  (a, qa): where on the read and
 *                         on the strand a maximal exact match starts (a < rlen, qa < tlen; the base before it does not agree
 *                         or is outside the overlap).  out[0] = 1 if no run of K agreeing bases lies left of it on its
 *                         diagonal (this match owns the alignment); out[1], out[2] = the overlap [x_lo, x_hi) in read
 *                         offsets; out[3] = its non-agreeing positions.  VS_E_ARG: a NULL text, K = 0, a or qa outside. */
int vs_pileup_layout(vs_ctx *ctx, uint32_t *d_first, uint64_t *n_slots);
int vs_node_pileup(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t *d_diff, uint64_t *d_alt, uint32_t max_mismatch,
                   uint64_t *d_tally);
int vs_pileup_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound,
                   uint64_t plan[8]);
int vs_pileup_scan_host(const uint32_t *read_words, const uint32_t *read_mask, const uint32_t *strand_words, uint32_t rlen, uint32_t tlen, uint32_t a,
                        uint32_t qa, uint32_t K, uint32_t out[4]);

/* ---- which variant sites travel together on one read pair (additions to ABI 11 without a new number: nothing that exists
 * changes) --  No counterpart in the reference.  A SITE is a position p of a segment n with len_n >= K = k + 1, given as its
 * pileup slot first[n] + p (vs_pileup_layout); the site list is an ascending array of distinct slots.  A FRAGMENT is the two
 * ends 2p and 2p + 1 of a block (in a singles block the one present end).  Every alignment the pileup credits (anchored, once
 * per diagonal, at most max_mismatch non-agreeing positions in its overlap, both strands) makes one RAW observation (site, c)
 * for every site under its overlap, c the read's byte there as it reads on the forward strand (0..3 = ACGT, complemented on
 * the reverse-complement strand, 4 = a byte outside ACGT): the column rule of alt, taken at agreeing positions too.  A
 * fragment with more than 32 raw observations over both ends is OVERFLOW and deposits nothing.  Otherwise it OBSERVES (s, c)
 * once if every raw observation it holds of site s carries the same c; else s is DISCORDANT for it and left out.  Every pair
 * s < t of observed sites on one segment with pos_t - pos_s <= span adds 1 to the cell of (s, t) at [c_s][c_t]; a pair on two
 * segments or further apart is UNSTORED.  tests/site_pairs_model.py states it; csrc/vs_site_pairs_plan.h has the launch and
 * the rows, csrc/vs_site_pairs_core.h what a lane does.
 *   vs_site_pairs_rows_host : host only, no device, a pure function.  (seg[i], pos[i]), i < n_sites: the sites, strictly
 *                             ascending by segment (the index's own numbering), then position.  row_first: n_sites + 1
 *                             words, written: the cells before every site's and all of them behind; site i's partners are
 *                             the later sites of its segment within span, contiguous behind it, so the cell of (s, t) is
 *                             row_first[s] + (t - s - 1).  *n_cells = the total.  VS_E_ARG: not ascending; VS_E_RANGE: 2^29
 *                             sites or more (an entry is site << 3 | c) or 2^32 cells or more: lower the span.
 *   vs_site_pairs_plan      : host only, a pure function: plan[0] = 1 if k_node_site_pairs is launched (0: no end holds K
 *                             bases); [1] = workgroups; [2] = ends per workgroup, a multiple of 64, so that no workgroup
 *                             and no batch of 64 ends cuts a pair; [3..5] = 0; [6] = LDS bytes per workgroup; [7] = threads
 *                             per workgroup.  VS_E_ARG: an odd n_ends; VS_E_RANGE: more than 2^25 - 2 nodes, 2^32 ends.
 *   vs_site_pairs_frag_host : host only, no device: the reduction the kernel runs on one fragment's list
 *                             (csrc/vs_site_pairs_core.h) on HOST buffers.  raw: n <= 32 entries site << 3 | c in any order;
 *                             kept: room for 32, written with the observations, ascending; out[0] = how many, out[1] = the
 *                             discordant sites.  VS_E_ARG: n > 32.
 *   vs_node_site_pairs      : one block through k_node_site_pairs on the context's current index.  d_first: what
 *                             vs_pileup_layout wrote for THIS index; d_site_slot: DEVICE, n_sites uint32 ascending;
 *                             d_row_first: DEVICE, n_sites + 1 uint32 as vs_site_pairs_rows_host made them; d_cells: DEVICE,
 *                             row_first[n_sites] x 25 uint64, zero before the first block, added to with one atomic per
 *                             stored pair; d_tally: DEVICE, 5 uint64, added to: fragments with a raw observation, overflow
 *                             fragments, discordant (fragment, site) incidences, pairs stored, pairs unstored.  Enqueued on
 *                             the ctx stream; with n_sites == 0 nothing is launched.  Blocks must have been built after
 *                             vs_ctx_keep_masks(ctx, 1).  VS_E_ARG: an odd number of ends; VS_E_RANGE: 2^29 sites. */
int vs_site_pairs_rows_host(const uint32_t *seg, const uint32_t *pos, uint64_t n_sites, uint32_t span, uint32_t *row_first, uint64_t *n_cells);
int vs_site_pairs_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t plan[8]);
int vs_site_pairs_frag_host(const uint32_t *raw, uint32_t n, uint32_t *kept, uint32_t out[2]);
int vs_node_site_pairs(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, const uint32_t *d_site_slot, uint32_t n_sites,
                       const uint32_t *d_row_first, uint64_t *d_cells, uint32_t max_mismatch, uint64_t *d_tally);

/* ---- the pileup kept apart by strand, and its records found on the device (additions to ABI 11 without a new number:
 * nothing that exists changes) --  No counterpart in the reference.  Everything the base pileup above defines holds unchanged;
 * the PLANE of a credited alignment is its strand t: plane 0 -- the end's bytes, as the ingest delivers them, read along the
 * segment's forward text; plane 1 -- read along its reverse complement (not the mate number, not the end's parity).  For
 * every overlap position depth[n][p][t] += 1, and where it does not agree alt[n][p][t][c] += 1, c as before.  Summed over t
 * both tables are the base pileup's exactly and the two tallies are equal; a palindromic overlap puts 1 into each plane; a read
 * and its reverse complement put the same forward-strand column into different planes.  RECORDS, for one position with the
 * segment's base ref: count[t][b] = alt[t][b] for b != ref and count[t][ref] = depth[t] - the five alt columns of t; DP = the
 * sum of count over both planes and A, C, G, T (`other` is left out); for b != ref in ACGT order AD = count[0][b] +
 * count[1][b], and b is a record when AD > 0, AD >= min_alt_count and (double)AD >= min_alt_frac * (double)DP, one IEEE double
 * product compared as it stands (0.07 * 100 > 7: no record; 0.29 * 100 <= 29: one).  A record carries DP4 = ref_f, ref_r,
 * alt_f, alt_r = count[0][ref], count[1][ref], count[0][b], count[1][b]; with min_alt_strand >= 1 it FAILS the strand filter
 * when alt_f or alt_r is below it, and stays a record.  tests/strand_pileup_model.py states all of it;
 * csrc/vs_pileup_call_core.h is the rule of one position.  Six uint64 make a record: slot << 5 | strand_fail << 4 | ref << 2 |
 * alt (2-bit base codes), then DP, ref_f, ref_r, alt_f, alt_r.
 *   vs_node_pileup_strands : one block through k_node_pileup_strands on the context's current index: vs_node_pileup with the
 *                            planes kept apart.  n_slots: the S vs_pileup_layout gave for THIS index; d_diff: DEVICE, 2 x S
 *                            uint32, plane-major, zero before the first block -- each plane is a difference array with its own
 *                            sentinels and is folded on its own by vs_cover_fold (S slots at d_diff + t * S into S uint64 at
 *                            d_depth + t * S); d_alt: DEVICE, S x 2 x 5 uint64 [slot][plane][column], zero before the first
 *                            block; d_tally as vs_node_pileup's.  The fold rule is vs_pileup_plan's, unchanged: one end adds
 *                            at most its length to one slot of one plane.  Enqueued on the ctx stream.  Blocks must have been
 *                            built after vs_ctx_keep_masks(ctx, 1).  VS_E_RANGE as vs_node_pileup, and S >= 2^32.
 *   vs_pileup_call         : the records of all S slots, found by two passes with one lane per slot and the exclusive scan
 *                            between them; the segment's base comes from the index's own forward text, a sentinel slot emits
 *                            nothing and is not read.  planes = 2: d_depth [2][S], d_alt [S][2][5] as above; planes = 1: the
 *                            tables of vs_node_pileup, d_depth [S], d_alt [S][5], folded -- then ref_r = alt_r = 0.  *n (host)
 *                            = the exact number of records.  With cap >= *n they are written to d_out (DEVICE, cap x 6 uint64)
 *                            ascending by slot, then alt base; with cap < *n NOTHING is written and the call returns VS_OK:
 *                            allocate *n records and call again.  Synchronises the ctx stream.  Uses 4 bytes per slot of the
 *                            context's scratch, shared with vs_cover_fold.  VS_E_ARG: a NULL pointer, planes outside {1, 2},
 *                            min_alt_frac NaN or negative, min_alt_strand != 0 with one plane; VS_E_RANGE: 2^32 slots or
 *                            records.
 *   vs_pileup_call_host    : host only, no device: the rule of csrc/vs_pileup_call_core.h, the code both passes run, on ONE
 *                            position.  ref: 0..3; depth: `planes` uint64; alt: planes x 5 uint64; out: room for three
 *                            records, written with *n of them (their slot is 0).  VS_E_ARG as vs_pileup_call, and ref > 3. */
int vs_node_pileup_strands(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint64_t n_slots, uint32_t *d_diff, uint64_t *d_alt,
                           uint32_t max_mismatch, uint64_t *d_tally);
int vs_pileup_call(vs_ctx *ctx, const uint32_t *d_first, uint64_t n_slots, uint32_t planes, const uint64_t *d_depth, const uint64_t *d_alt,
                   uint64_t min_alt_count, double min_alt_frac, uint64_t min_alt_strand, uint64_t *d_out, uint64_t cap, uint64_t *n);
int vs_pileup_call_host(uint32_t ref, uint32_t planes, const uint64_t *depth, const uint64_t *alt, uint64_t min_alt_count, double min_alt_frac,
                        uint64_t min_alt_strand, uint64_t out[3][6], uint32_t *n);

/* ---- insertions and deletions of the reads against the segments (additions to ABI 11 without a new number: nothing that
 * exists changes) --  No counterpart in the reference.  With K = k + 1 and a maximum length G (1 <= G <= 32): R is a read end as
 * the ingest delivers it, T a strand t of a segment n with len_n >= K, (a, qa, len) a maximal exact match of R with T of at
 * least K agreeing bases -- the match the base pileup is handed, with its guard qa + len <= len_n.  The match is TESTED when
 * a > 0 and qa > 0: its left neighbour lies inside both texts and does not agree.  The candidates are tried in the order
 * deletion 1, insertion 1, deletion 2, ... deletion G, insertion G; the first that holds is the event, a match yields at most
 * one.  DELETION of L: a >= K and qa >= L + K, and R[a-K .. a) agrees with T[qa-L-K .. qa-L) (the pileup's rule: a byte
 * outside ACGT does not agree); the strand's bases [qa-L, qa) are missing from the read.  INSERTION of L: a >= L + K and
 * qa >= K, and R[a-L-K .. a-L) agrees with T[qa-K .. qa); I = R[a-L .. a) stands before strand position qa; if I holds a byte
 * outside ACGT the event is dropped and tallied and no further candidate is tried.  NORMALISATION, F the segment's forward
 * text: on strand 1 a deletion of [s, s+L) is forward [len_n-s-L, len_n-s) and an insertion of I before s is revcomp(I) before
 * len_n - s; then a deletion (u, L) moves to u - 1 while u > 0 and F[u-1] == F[u+L-1], an insertion (u, I) becomes (u - 1,
 * F[u-1] + I[:-1]) while u > 0 and F[u-1] == I[-1].  The PLANE of an event is t.  An event is two uint64: w0 = slot << 8 |
 * plane << 7 | kind << 6 | (L - 1), slot = first[n] + u on vs_pileup_layout's layout, kind 0 a deletion, 1 an insertion; w1 =
 * the inserted bases on the forward strand, 2 bits each, the first lowest, 0 for a deletion.  Per end and per strand: two mates
 * over one event are two events.  tests/indel_model.py states all of it; csrc/vs_indel_core.h is the code of one match.
 *   vs_node_indels     : one block through k_node_indels on the context's current index, launched by vs_pileup_plan's plan.
 *                        d_first: what vs_pileup_layout wrote; max_len: G; d_events: DEVICE, cap x 2 uint64, in no order.  *n
 *                        (host) = the exact number of events of the block; with *n > cap the buffer's content is undefined:
 *                        call again with room for *n.  d_tally: DEVICE, four uint64, ADDED to only by a call that fit: matches
 *                        tested, deletions, insertions, insertions dropped.  Synchronises the ctx stream (the addition to
 *                        d_tally is enqueued behind it).  Blocks must have been built after vs_ctx_keep_masks(ctx, 1).
 *                        VS_E_ARG: a NULL pointer, max_len outside 1..32; VS_E_RANGE as vs_node_pileup.
 *   vs_indel_scan_host : host only, no device: the code a lane runs, on ONE match of a read (packed words, mask or NULL) with
 *                        a strand (its packed words, and the segment's packed forward text), every array with three zero words
 *                        behind its last.  out[0]: 0 not tested, 1 tested without an event, 2 an event, 3 dropped; out[1] =
 *                        kind << 8 | L (2, 3); out[2] = u and out[3] = w1 (2).  VS_E_ARG: a NULL pointer, K == 0, G outside
 *                        1..32, strand > 1, a >= rlen, qa >= tlen. */
int vs_node_indels(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t max_len, uint64_t *d_events, uint64_t cap, uint64_t *n,
                   uint64_t *d_tally);
int vs_indel_scan_host(const uint32_t *read_words, const uint32_t *read_mask, const uint32_t *strand_words, const uint32_t *fwd_words, uint32_t rlen,
                       uint32_t tlen, uint32_t strand, uint32_t a, uint32_t qa, uint32_t K, uint32_t G, uint64_t out[4]);

/* Testing aid (ABI 11): the two exclusive scans under the index build, the locus sort, every row_ptr and every member,
 * record and word offset, run alone on values the caller made up, launched exactly as their callers launch them (no kernel
 * of its own).  HOST pointers: in[n + guard] = the n values and behind them `guard` words of a sentinel the caller chose;
 * out[n + guard] = the device buffer the scan wrote, whole: out[i] = in[0] + .. + in[i - 1] mod 2^32 for i < n, and the
 * sentinel words as they were handed in unless the scan wrote past its end.
 *   which = 0 : the three-launch scan of any length (2 048 values per workgroup, the block sums walked 256 at a time), its
 *               scratch sized ceil(n / 2048) + 1 words as its callers size it.  flags bit 0: in place (out == in on the
 *               device); otherwise the first n words of the device's out hold 0xA5A5A5A5 before the scan.  flags bit 1:
 *               the scan gets no place for its total, and *total (may be NULL then) is left as it was; otherwise *total =
 *               the exact 64-bit sum, 0 for n = 0.
 *   which = 1 : the one-workgroup scan of the streamed ingests (1 024 threads, a slice of ceil(n / 1024) values each):
 *               always in place, n < 2^32, flags bit 1 is VS_E_ARG; *total = the sum mod 2^32 (its callers' totals stay
 *               below 2^32).
 * The device's word for the total holds all ones before either scan. */
int vs_scan_check(vs_ctx *ctx, int which, const uint32_t *in, uint64_t n, int flags, uint32_t *out, uint64_t guard,
                  uint64_t *total);

/* ---- graph stages: K5 PE-link table ---------------------------------------------------------
 * Replaces process_pe_info (utils/VStrains_IO.py:598-627) and every later read or rewrite of the
 * pe_info dict (utils/VStrains_Decomposition.py:141-143,178,273,492-503,608-617,672-684;
 * utils/VStrains_Utilities.py:488-499; utils/VStrains_Extension.py:62,766-799).
 * The table is P0[i][j] = node[i][j] + node[j][i] + short[i][j] + short[j][i] for i != j and
 * P0[i][i] = node[i][i] + short[i][i], int64, resident on the device; it is never rewritten:
 * a lookup for nodes made by splits / contractions is a sum over two lists of original rows
 * (see vstrains_amd/graph/ops.py for the equivalence, tests/test_graph_golden.py for the check
 * against the literal dict). */
typedef struct vs_links vs_links;
/* d_node_mat / d_short_mat: DEVICE pointers to the N*N uint32 counters vs_pe_count filled. */
int vs_links_from_counts(vs_ctx *ctx, const uint32_t *d_node_mat, const uint32_t *d_short_mat,
                         uint32_t n, vs_links **out);
/* ABI 10: the same from counters that keep a dirty-tile map (vs_pe_count_tracked: one byte per 64 x 64 tile of node_mat, then of
 * short_mat; a cell outside the marked tiles is zero).  From `sparse_min_nodes` nodes on (0 = the default, 32 768) the table
 * is held as CSR rows of its non-zero cells, built from the marked tiles only -- 0.4 GB instead of 23.7 GB at 54 465 nodes, and
 * no pass over the counters; below, or without a map, exactly vs_links_from_counts.  Every vs_links_* call takes either form.
 * (process_pe_info, IO.py:598-627: a dict of N (N + 1) / 2 keys in the reference.) */
int vs_links_from_counts_tracked(vs_ctx *ctx, const uint32_t *d_node_mat, const uint32_t *d_short_mat, uint32_t n,
                                 const uint8_t *d_tile_map, uint32_t sparse_min_nodes, vs_links **out);
/* Same from DEVICE int64 totals (vs_counts_fold). */
int vs_links_from_wide(vs_ctx *ctx, const int64_t *d_node_mat, const int64_t *d_short_mat,
                       uint32_t n, vs_links **out);
/* Same from HOST int64 matrices (e.g. parsed back from pe_info / st_info text). */
int vs_links_from_host(vs_ctx *ctx, const int64_t *node_mat, const int64_t *short_mat, uint32_t n,
                       vs_links **out);
/* (addition to ABI 10) The same table from cells (HOST arrays; vs_info_parse of both files, one after the other): what
 * vs_links_from_host gives for dense matrices built by m[r][c] += v -- a cell with r != c adds v to P0[r][c] and to P0[c][r],
 * one with r == c adds v to P0[r][r]; duplicates add.  Below `sparse_min_nodes` nodes (0 = 32 768, as above) the table is
 * dense: the cells are uploaded and scattered into a zeroed table by a kernel; from there on it is the CSR form (row_ptr u32,
 * col u32 ascending, val i64, non-zero sums only), mirrored, sorted and merged on the host threads and uploaded.  A cell
 * outside n x n is VS_E_RANGE. */
int vs_links_from_cells(vs_ctx *ctx, const uint32_t *rows, const uint32_t *cols, const int64_t *vals, uint64_t n_cells, uint32_t n,
                        uint32_t sparse_min_nodes, vs_links **out);
/* (addition to ABI 10) The same table straight from the two files, read where the table lives.  A file that is BGZF from its
 * first byte to its last (what vs_write_info_bgzf writes) is uploaded compressed, window by window, and inflated on the device
 * (one wavefront per member, CRC checked); a plain file is uploaded window by window from the mapped file; the text of a window
 * (window_bytes, 0 = 256 MB; a buffer always begins at a line start, the cut line is carried) is scanned and parsed by kernels
 * and every non-zero count is added into ONE zeroed table (the buffer of vs_links_reserve when there is one) by 64-bit atomic
 * adds -- or, from `sparse_min_nodes` nodes on, appended to a cell list that the CSR build of vs_links_from_cells takes.  No
 * text exists on the host.  Any other gzip file, a file with a line longer than a window, and a file with an error go through
 * vs_info_parse on the host, which words the error (VS_E_ARG, the same text in vs_last_error(ctx)).  When either file holds a
 * '\r' or a byte >= 0x80 the call returns 0 with *out = NULL and the flags set: the caller keeps its own loop, as after
 * vs_info_parse.  info, 8 words per file (pe_info first): [0] route -- 1 BGZF inflated on the device, 2 plain text parsed on the
 * device, 3 vs_info_parse --, [1] lines, [2] lines skipped for an unknown id, [3] lines that named two known ids, [4] members
 * inflated on the device, [5] text bytes, [6] windows, [7] flags as vs_info_parse's info[1]. */
int vs_links_from_info(vs_ctx *ctx, const char *pe_path, const char *st_path, const uint8_t *names, const uint64_t *name_off,
                       uint32_t n, uint32_t sparse_min_nodes, uint64_t window_bytes, vs_links **out, uint64_t info[16]);
/* Optional, ABI 9: set aside the device buffer of the next table of n nodes (n*n int64) now -- typically when the counters
 * are allocated, before any read is counted -- so that vs_links_from_counts / _from_wide / _from_host does not have to ask the
 * driver for it later (a hipMalloc of tens of gigabytes takes 0.3 ms or half a second depending on what the process freed
 * before: 23.7 GB at 54 465 nodes).  The buffer belongs to the context until a table of that size takes it; a second call
 * replaces it, n = 0 gives it back.  The reference has no counterpart: its table is a Python dict. */
int vs_links_reserve(vs_ctx *ctx, uint32_t n);
void vs_links_free(vs_ctx *ctx, vs_links *links);
int vs_links_size(const vs_links *links, uint32_t *n);
int vs_links_to_host(vs_ctx *ctx, const vs_links *links, int64_t *out /* n*n */);
/* A pool of index lists: list l is list_idx[list_off[l] .. list_off[l+1]) (rows of P0, repeats
 * allowed, may be empty).  out[q] = sum over r in list qa[q], c in list qb[q] of P0[r][c].
 * Host pointers. */
int vs_links_block_sums(vs_ctx *ctx, const vs_links *links, const uint64_t *list_off,
                        const uint32_t *list_idx, uint32_t n_lists, const uint32_t *qa,
                        const uint32_t *qb, uint64_t n_queries, int64_t *out);
/* out[g * n_groups + h] = block sum of group g x group h, for all pairs (final_link_info,
 * Extension.py:766-799).  Host pointers. */
int vs_links_group_matrix(vs_ctx *ctx, const vs_links *links, const uint64_t *list_off,
                          const uint32_t *list_idx, uint32_t n_groups, int64_t *out);
/* Testing aid (addition to ABI 11, like vs_index_export / vs_scan_check): the CSR rows of a table exactly as the device holds
 * them, so that a test sees what vs_links_to_host's dense answer hides -- the order of the columns inside a row, a column
 * stored twice, a stored zero, a row_ptr that does not end at nnz.  Copies only, no kernel.  HOST pointers: *nnz (may be NULL)
 * = the number of stored cells the table records; row_ptr (may be NULL) receives the n + 1 row offsets; col and val (both or
 * neither NULL) receive the first *nnz stored columns and values when cap >= *nnz -- a smaller cap is VS_E_RANGE, with *nnz
 * set, nothing else written.  A dense table is VS_E_ARG. */
int vs_links_export_csr(vs_ctx *ctx, const vs_links *links, uint32_t *row_ptr, uint32_t *col, int64_t *val, uint64_t cap,
                        uint64_t *nnz);

/* ---- graph stages: K6 vertex scan + chain ranking, K7 edge flow -------------------------------
 * One call per re-initialised stage graph (store_reinit_graph, VStrains_IO.py:630-642).
 * The graph is a CSR in adjacency order: row v = nbr/eidx[row_ptr[v] .. row_ptr[v+1]), its
 * first n_out[v] entries are out-edges (target, edge index), the rest in-edges (source, edge
 * index).  edge_black is indexed by edge index (n_edge_slots of them).  Host pointers; any
 * output pointer may be NULL.
 *   flow[e]        assign_edge_flow, VStrains_Utilities.py:14-31 (numpy.sum / numpy.mean order)
 *   nontrivial[v]  is_non_trivial, VStrains_Utilities.py:162-172
 *   fork_kind[v]   1: one black in / several black out, 2: several in / one out
 *                  (VStrains_Decomposition.py:715,763)
 *   chain_next[v]  target of v's simple out-edge or -1 (simp_path, VStrains_Utilities.py:398-402)
 *   chain_top[v], chain_rank[v]  head of v's chain of simple edges and v's distance from it
 *                  (pointer jumping; rank -1 on a ring of simple edges)
 *   *zero_sum_edge smallest edge index whose flow would divide by a zero neighbour sum, or
 *                  0xFFFFFFFF (the reference raises FloatingPointError there, vstrains:25) */
int vs_graph_refresh(vs_ctx *ctx, uint32_t n_vertices, uint32_t n_edge_slots,
                     const uint64_t *row_ptr, const uint32_t *n_out, const uint32_t *nbr,
                     const uint32_t *eidx, const double *dp, const uint8_t *vertex_black,
                     const uint8_t *edge_black, double *flow, uint8_t *nontrivial,
                     uint8_t *fork_kind, int32_t *chain_next, int32_t *chain_top,
                     int32_t *chain_rank, uint32_t *zero_sum_edge);

/* ---- graph stages: native stage handle ----------------------------------------------------------
 * The state the reference keeps in a graph_tool.Graph plus Python dicts and re-derives from a GFA file after every
 * pass -- graph, simp_node_dict, simp_edge_dict, contig_dict, the rewritten pe_info, full_link, usages -- as ONE
 * object in this library, with every stage of VStrains_SPAdes.py:140-248 as one call on it.  Flows, vertex scan and
 * chain ranking of each re-initialised graph and all PE-link sums run on the device (K5-K7 above); the decisions run
 * on the host inside the call; stage GFA files are written by worker threads of the handle and are complete when the
 * call that names them returns.  One entry per reference function:
 *   vs_stage_edge_cleaning          edge_cleaning, Decomposition.py:822-905
 *   vs_stage_reinit                 store_reinit_graph, IO.py:630-642
 *   vs_stage_disentangle            iter_graph_disentanglement, Decomposition.py:908-1042 (balance_split :91-530,
 *                                   trivial_split :533-688, simp_path_compactification Utilities.py:383-574,
 *                                   contig_dict_remapping :281-380, contig_dup_removed_s :589-616, trim_contig_dict :147-159)
 *   vs_stage_best_matching          best_matching, Extension.py:10-111
 *   vs_stage_increment_nt_coverage  increment_nt_branch_coverage, Utilities.py:183-208
 *   vs_stage_write_gfa              graph_to_gfa, IO.py:337-372
 *   vs_stage_path_extension         path_extension, Extension.py:484-899 (global_trivial_split Decomposition.py:691-819,
 *                                   contig_extension / final_extension Extension.py:115-418, reduce_graph :429-455)
 *   vs_stage_write_contigs          contig_dict_to_path IO.py:558-595 / contig_dict_to_fasta :518-536 of contig_dict
 * State crosses the boundary as byte blobs (vs_stage_import / vs_stage_export): a sequence of sections, each a
 * uint32 tag (VS_STAGE_*) and a payload of little-endian arrays and newline-joined string lists; the layout is stated
 * where it is written, vstrains_amd/graph/native_stage.py.  `links` must outlive the handle.  Errors: the return
 * code, and vs_stage_error for the message and the name of the exception the reference raises in that situation. */
typedef struct vs_stage vs_stage;
enum {
    VS_STAGE_GRAPH = 1,    /* vertices, adjacency rows, edge slots, free list, the two ordered maps */
    VS_STAGE_CONTIGS = 2,  /* contig_dict */
    VS_STAGE_LINKS = 4,    /* full_link (best_matching's result, consumed by path_extension) */
    VS_STAGE_STRAINS = 8,  /* strain_dict (export only) */
    VS_STAGE_USAGES = 16,  /* usages (export only) */
    VS_STAGE_LOG = 32,     /* the log lines of the calls since the last export of this section (export only) */
    VS_STAGE_SCAN = 64,    /* non-trivial branches, fork kinds, chain ranks of the last re-initialisation */
    VS_STAGE_ASSIGNED = 128 /* edge_cleaning's result: (source id, target id) -> accounted for (export only) */
};
int vs_stage_create(vs_ctx *ctx, const vs_links *links, vs_stage **out);
void vs_stage_destroy(vs_stage *st);
const char *vs_stage_error(const vs_stage *st, const char **kind);
int vs_stage_set_debug(vs_stage *st, int on); /* also collect the DEBUG lines */
/* names of the rows of `links`, '\n'-joined (the nodes of s_graph_L1 in the numbering the table was built in) */
int vs_stage_set_link_names(vs_stage *st, uint32_t n, const uint8_t *joined, uint64_t len);
int vs_stage_import(vs_stage *st, const uint8_t *blob, uint64_t len);
/* the buffer belongs to the handle and is valid until the next call on it */
int vs_stage_export(vs_stage *st, uint32_t what, const uint8_t **blob, uint64_t *len);
/* pe_info[(a, b)] as the dict the reference rewrites through every split / fork / contraction would hold it now */
int vs_stage_link(vs_stage *st, const char *a, const char *b, int64_t *out);
int vs_stage_edge_cleaning(vs_stage *st);
int vs_stage_reinit(vs_stage *st, const char *gfa_path);
/* scan of an imported graph without gray objects (the reference asks get_non_trivial_branches, Utilities.py:175-180,
 * of whatever graph it is handed); flows are left as they are */
int vs_stage_refresh_scan(vs_stage *st);
int vs_stage_disentangle(vs_stage *st, double threshold, const char *temp_dir);
int vs_stage_best_matching(vs_stage *st);
int vs_stage_increment_nt_coverage(vs_stage *st);
int vs_stage_write_gfa(vs_stage *st, const char *path);
int vs_stage_write_contigs(vs_stage *st, const char *paths_file, const char *fasta_file); /* either may be NULL */
int vs_stage_path_extension(vs_stage *st, double threshold, const char *temp_dir);
/* VStrains_SPAdes.py:251-262 on the strain records path_extension left: contig_resolve (Utilities.py:211-224),
 * trim_contig_dict (:147-159) measured on the graph kept by vs_stage_keep_graph -- call it right after the
 * es_graph_L2 re-initialisation --, contig_dup_removed_s (:589-616), tmp/tmp_strain.paths (IO.py:558-595) */
int vs_stage_keep_graph(vs_stage *st);
int vs_stage_finish_strains(vs_stage *st, const char *tmp_paths_file);
/* numpy.median of the vertex depths (the thresholds of VStrains_SPAdes.py:187,237 are 0.05 x this) */
int vs_stage_median_depth(vs_stage *st, double *out);
/* info[0] re-initialisations, [1] of which reused an untouched state, [2] flow/scan launches, [3] link-sum launches,
 * [4] files written, [5] bytes written, [6] vertices, [7] live edges; secs[0] in re-initialisations, [1] of which in
 * the flow/scan operation, [2] in link sums, [3] busy time of the file writers */
int vs_stage_counters(vs_stage *st, uint64_t info[8], double secs[4]);
/* "name=seconds;" per section of the stage calls so far (where a leg's time goes), into buf */
int vs_stage_sections(vs_stage *st, char *buf, uint64_t cap);

/* ---- device memory helpers for C callers without another allocator ----------------------- */
int vs_dev_alloc(vs_ctx *ctx, size_t bytes, void **out); /* zero-filled */
int vs_dev_free(vs_ctx *ctx, void *ptr);
int vs_dev_zero(vs_ctx *ctx, void *ptr, size_t bytes);
int vs_dev_to_host(vs_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VSTRAINS_HIP_H */
