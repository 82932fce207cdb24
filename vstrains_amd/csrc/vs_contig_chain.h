// Contigs threaded through the graph, the host half: the maximal exact matches k_contig_mems (vs_pe.hip) found, chained into
// the parts and signed tokens of a SPAdes .paths entry.  ONE pure function over plain arrays, in the style of vs_depth_plan.h
// and vs_pe_pack.h: a host compiler takes this header as it is and no device is needed.
//
// The rule (tests/contig_thread_model.py states it window by window, over strings).  With K = k + 1, window i of a contig is
// c[i : i + K]; its hits are the (segment, strand, pos) at which a strand's text holds it.  Left to right: CONTINUE on
// (n, s, p + 1) if that is a hit; else CROSS, when p was the segment's last window, to the smallest (segment, strand) that
// hits at pos 0 -- a new token; else open a NEW PART at the smallest (segment, strand, pos); a window without hits ends
// the part.  A match record stands for the run of hits on one diagonal of one strand, maximal both ways, so:
//   continue = stay in the record to its last window, end = off + len - K;
//   cross    = the record ends at its segment's end, and a record B has B.off == end + 1 and B.pos == 0;
//   new part = the smallest (segment, strand, pos at that window) over the records that cover the window;
//   records wholly inside windows already chosen are never looked at again.
#ifndef VS_CONTIG_CHAIN_H
#define VS_CONTIG_CHAIN_H
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#define VS_MEM_WORDS 5u  // a match record, five words (32 + 24 + 26 + 24 + 24 bits do not fit four)
struct VsMem {
    uint32_t contig;  // the block's read (a singles block) or end
    uint32_t off;     // first base of the match in the contig
    uint32_t seg;     // segment | strand << 31 (strand 1: the match is on the segment's reverse complement)
    uint32_t pos;     // first base of the match in that strand's text
    uint32_t len;     // bases, >= K
};
#define VS_TOKEN_WORDS 4u
struct VsChainToken {
    uint32_t contig;
    uint32_t seg;      // segment | strand << 31
    uint32_t windows;  // windows of the contig this token was chosen for
    uint32_t first;    // 1: the token opens a part
};

inline uint64_t vs_mem_segkey(const VsMem &m) { return ((uint64_t)(m.seg & 0x7FFFFFFFu) << 1) | (m.seg >> 31); }  // orders (segment, strand)

// mems: any order, sorted here.  seg_len[segment] in bases.  tokens: appended in contig order; ambiguous[contig] += the
// windows of that contig with more than one hit.  The caller has checked contig < n_contigs, segment < n_segs, len >= K.
inline void vs_contig_chain_for(std::vector<VsMem> &mems, const uint32_t *seg_len, uint32_t K, std::vector<VsChainToken> &tokens,
                                uint64_t *ambiguous) {
    std::sort(mems.begin(), mems.end(), [](const VsMem &a, const VsMem &b) {
        if (a.contig != b.contig) return a.contig < b.contig;
        if (a.off != b.off) return a.off < b.off;
        const uint64_t ka = vs_mem_segkey(a), kb = vs_mem_segkey(b);
        if (ka != kb) return ka < kb;
        return a.pos < b.pos;
    });
    const size_t n = mems.size();
    std::vector<size_t> active;
    std::vector<std::pair<uint64_t, int>> events;
    auto end_of = [&](size_t x) { return (uint64_t)mems[x].off + mems[x].len - K; };  // the record's last window
    for (size_t a = 0; a < n;) {
        size_t b = a;
        while (b < n && mems[b].contig == mems[a].contig) b++;
        // windows under more than one record
        events.clear();
        for (size_t x = a; x < b; x++) {
            events.emplace_back((uint64_t)mems[x].off, 1);
            events.emplace_back(end_of(x) + 1u, -1);
        }
        std::sort(events.begin(), events.end());
        int64_t depth = 0;
        for (size_t x = 0; x + 1 < events.size(); x++) {
            depth += events[x].second;
            if (depth > 1) ambiguous[mems[a].contig] += events[x + 1].first - events[x].first;
        }
        // the walk
        active.clear();
        size_t next = a;
        uint64_t i = 0;
        bool have = false, first = true;
        size_t cur = 0;
        for (;;) {
            while (next < b && mems[next].off <= i) active.push_back(next++);
            if (!have) {
                size_t kept = 0;
                for (size_t x : active)
                    if (end_of(x) >= i) active[kept++] = x;
                active.resize(kept);
                if (active.empty()) {
                    if (next == b) break;
                    i = mems[next].off;
                    continue;
                }
                cur = active[0];
                for (size_t x : active) {
                    const uint64_t kx = vs_mem_segkey(mems[x]), kc = vs_mem_segkey(mems[cur]);
                    const uint64_t px = mems[x].pos + (i - mems[x].off), pc = mems[cur].pos + (i - mems[cur].off);
                    if (kx < kc || (kx == kc && px < pc)) cur = x;
                }
                first = true;
            }
            const VsMem A = mems[cur];
            tokens.push_back(VsChainToken{A.contig, A.seg, (uint32_t)(end_of(cur) - i + 1u), first ? 1u : 0u});
            i = end_of(cur) + 1u;
            have = false;
            if (A.pos + A.len == seg_len[A.seg & 0x7FFFFFFFu]) {
                while (next < b && mems[next].off <= i) active.push_back(next++);
                for (size_t x : active)
                    if (mems[x].off == i && mems[x].pos == 0u && (!have || vs_mem_segkey(mems[x]) < vs_mem_segkey(mems[cur]))) {
                        cur = x;
                        have = true;
                    }
                first = false;
            }
        }
        a = b;
    }
}

#endif  // VS_CONTIG_CHAIN_H
