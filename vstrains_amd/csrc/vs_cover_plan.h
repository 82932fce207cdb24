// The plan of one block of the depth profile (vs_node_cover): the launch of k_node_cover (vs_pe.hip) and the rule by which
// the difference array is folded into the 64-bit totals (vs_cover_fold), as ONE pure function of scalars, in the style of
// vs_depth_plan.h.  Plain C++: a host compiler takes this header as it is.
//
// What the pass computes.  With K = k + 1, cov[n][p] for 0 <= p <= len_n - K is the number of triples (read end e, read
// offset i, table entry (n, p)) such that end_e[i : i + K] is a key of the reference's (k+1)-mer table
// (PE_Inference.py:117-135, oracle/pe_oracle.py:build_table) holding that entry: the triples KC[n] counts (vs_depth_plan.h),
// kept apart by the forward offset of their entry.  The value belongs to the WINDOW that starts at p: k-mer coverage, not
// base coverage.
//
// Slots.  Segment n owns len_n - K + 2 slots when len_n >= K, else none: one per window and ONE sentinel behind them.  A
// maximal match over windows p0 .. p1 adds +1 to slot p0 and -1 to slot p1 + 1 of a uint32 array (wrap-around adds); the
// -1 of a match flush with the segment's end lands in the sentinel, so every segment's slots sum to 0 and one plain
// exclusive scan over all slots, plus the slot's own word, is the coverage.
//
// The fold.  The scan is taken mod 2^32, so between two folds the true value of a slot must stay below 2^32.  One end adds
// at most 2 * (len_e - K + 1) to one slot (a window repeated all along the end, on a palindromic entry), so a block of
// n_ends ends of at most max_len bases weighs n_ends * 2 * (max_len - K + 1), and a fold is due BEFORE a block whose weight,
// added to the weight pending since the last fold, could reach the bound.
#ifndef VS_COVER_PLAN_H
#define VS_COVER_PLAN_H
#include <stdint.h>
#include <stdio.h>

#include "../../include/vstrains_hip.h"

#define COVER_TPB 1024u        // threads of a k_node_cover workgroup: sixteen wavefronts, each working through batches of 64 ends
#define COVER_WAVES (COVER_TPB / 64u)
// LDS words of one wavefront: the scan of its 64 ends' probe counts [65], the scan of 64 probes' posting counts [65], the
// probes' payloads and (end, read offset) [3 x 64] (rounded up to 16 bytes)
#define COVER_WAVE_WORDS 324u
#define COVER_HEAD_WORDS 4u    // the workgroup's batch counter (and three words of alignment)
#define COVER_LDS_WORDS (COVER_HEAD_WORDS + COVER_WAVES * COVER_WAVE_WORDS)
#define COVER_MIN_ENDS (64u * COVER_WAVES)  // a workgroup's share is at least one batch per wavefront
#define COVER_MAX_ENDS (1u << 31)           // ... and its batch counter (32 bits, sixteen wavefronts overshoot by 64 each) cannot wrap
#define COVER_BOUND (1ull << 32)            // what a slot must stay below between two folds

struct CoverPlan {
    int status;  // VS_OK, or VS_E_RANGE with msg
    char msg[128];
    uint32_t launch;       // 0: nothing is launched (no ends, or no end holds a window)
    uint32_t grid;         // workgroups
    uint64_t ends_per_wg;  // workgroup g takes ends [g * ends_per_wg, (g + 1) * ends_per_wg)
    uint64_t weight;       // the most this block can add to one slot: n_ends * 2 * (max_len - K + 1)
    uint32_t fold_first;   // 1: fold before this block is counted
    uint64_t pending;      // the weight pending once the block is counted
};

// n_nodes, K: the index; n_ends, max_len: the block; n_cu: compute units of the device; pending: the weight counted since
// the last fold; bound: what pending may not reach (0: COVER_BOUND; at most COVER_BOUND)
inline CoverPlan vs_cover_plan_for(uint32_t n_nodes, uint32_t K, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound) {
    CoverPlan p = {};
    p.pending = pending;
    if (!bound) bound = COVER_BOUND;
    if (bound > COVER_BOUND || pending >= COVER_BOUND) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "a fold bound or a pending weight beyond 2^32");
        return p;
    }
    if (n_nodes > 0x01FFFFFEu) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "more than 2^25-2 nodes");
        return p;
    }
    if (n_ends > 0xFFFFFFF0ull) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "a block of 2^32 ends or more");
        return p;
    }
    if (!n_ends || !n_nodes || !K || max_len < K) return p;  // no end holds a (k+1)-window: nothing pends either
    const uint64_t span = (uint64_t)max_len - K + 1u;  // (at most 2^32)
    const bool fits = n_ends <= (COVER_BOUND - 1u) / (2u * span);  // n_ends * 2 * span < 2^32, without forming a product that could wrap
    p.weight = fits ? n_ends * 2u * span : COVER_BOUND;
    if (!fits) {  // no fold can help inside one launch, whatever the bound asked for
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "%llu ends of up to %u bases could put 2^32 on one window: give the block in parts",
                 (unsigned long long)n_ends, max_len);
        return p;
    }
    p.fold_first = pending && pending + p.weight >= bound ? 1u : 0u;
    p.pending = (p.fold_first ? 0u : pending) + p.weight;
    // two workgroups of 1 024 threads per CU (22 KB of LDS each), as k_node_depth
    const uint64_t slots = (uint64_t)(n_cu ? n_cu : 1u) * 2u;
    uint64_t per = (n_ends + slots - 1u) / slots;
    if (per < COVER_MIN_ENDS) per = COVER_MIN_ENDS;
    if (per > COVER_MAX_ENDS) per = COVER_MAX_ENDS;
    p.ends_per_wg = per;
    p.grid = (uint32_t)((n_ends + per - 1u) / per);  // (at most 2^22: n_ends < 2^32, per >= 1 024)
    p.launch = 1u;
    return p;
}

#endif  // VS_COVER_PLAN_H
