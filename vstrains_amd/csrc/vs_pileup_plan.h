// The plan of one block of the base pileup (vs_node_pileup): the launch of k_node_pileup (vs_pe.hip) and the rule by which
// the depth's difference array is folded into the 64-bit totals (vs_cover_fold), as ONE pure function of scalars, with the
// shape and the fields of vs_cover_plan.h.  Plain C++: a host compiler takes this header as it is.
//
// What the pass computes.  With K = k + 1 and a mismatch budget M: an ALIGNMENT is a read end e laid along a strand t of a
// segment n (len_n >= K) on a diagonal d = strand offset - read offset; its overlap is the read offsets x with
// 0 <= x < len_e and 0 <= x + d < len_n.  A position agrees when the read byte is one of ACGT and equals the strand's base.
// The alignment is anchored when its overlap holds K agreeing positions in a row, and credited when it is anchored and at
// most M positions of its overlap do not agree.  A credited alignment adds 1 to depth[n][p] for every position p of its
// overlap, and 1 to alt[n][p][c] where it does not agree (c: the read's base on the forward strand, 4 for a byte outside
// ACGT): base coverage (tests/pileup_model.py).
//
// Slots.  Segment n owns len_n + 1 slots when len_n >= K, else none: one per position and ONE sentinel behind them.  A
// credited alignment over positions p0 .. p1 adds +1 to slot p0 and -1 to slot p1 + 1 of a uint32 array (wrap-around adds);
// the -1 of an overlap flush with the segment's end lands in the sentinel, so every segment's slots sum to 0 and one plain
// exclusive scan over all slots, plus the slot's own word, is the depth.  alt is counted in 64 bits and never folded.
//
// The fold.  The scan is taken mod 2^32, so between two folds the true value of a slot must stay below 2^32.  Through one
// position of a strand there is one diagonal per read offset, so one end has at most len_e alignments per strand covering a
// position, and two strands: it adds at most 2 * len_e to one slot.  A block of n_ends ends of at most max_len bases weighs
// n_ends * 2 * max_len, and a fold is due BEFORE a block whose weight, added to the weight pending since the last fold, could
// reach the bound.  The stranded pileup (vs_node_pileup_strands) keeps the two strands in two difference arrays and folds by
// this same plan: one end adds at most len_e to a slot of ONE plane, below the 2 * len_e assumed here.
#ifndef VS_PILEUP_PLAN_H
#define VS_PILEUP_PLAN_H
#include <stdint.h>
#include <stdio.h>

#include "../../include/vstrains_hip.h"

#define PILEUP_TPB 1024u       // threads of a k_node_pileup workgroup: sixteen wavefronts, each working through batches of 64 ends
#define PILEUP_WAVES (PILEUP_TPB / 64u)
// LDS words of one wavefront, as k_node_cover's: the scan of its 64 ends' probe counts [65], the scan of 64 probes' posting
// counts [65], the probes' payloads and (end, read offset) [3 x 64] (rounded up to 16 bytes)
#define PILEUP_WAVE_WORDS 324u
#define PILEUP_HEAD_WORDS 4u   // the workgroup's batch counter (and three words of alignment)
#define PILEUP_LDS_WORDS (PILEUP_HEAD_WORDS + PILEUP_WAVES * PILEUP_WAVE_WORDS)
#define PILEUP_MIN_ENDS (64u * PILEUP_WAVES)  // a workgroup's share is at least one batch per wavefront
#define PILEUP_MAX_ENDS (1u << 31)            // ... and its batch counter (32 bits, sixteen wavefronts overshoot by 64 each) cannot wrap
#define PILEUP_BOUND (1ull << 32)             // what a slot must stay below between two folds
#define PILEUP_ALT 5u                         // columns of alt: A C G T and `other`

struct PileupPlan {
    int status;  // VS_OK, or VS_E_RANGE with msg
    char msg[128];
    uint32_t launch;       // 0: nothing is launched (no ends, or no end holds K bases)
    uint32_t grid;         // workgroups
    uint64_t ends_per_wg;  // workgroup g takes ends [g * ends_per_wg, (g + 1) * ends_per_wg)
    uint64_t weight;       // the most this block can add to one slot: n_ends * 2 * max_len
    uint32_t fold_first;   // 1: fold before this block is counted
    uint64_t pending;      // the weight pending once the block is counted
};

// n_nodes, K: the index; n_ends, max_len: the block; n_cu: compute units of the device; pending: the weight counted since
// the last fold; bound: what pending may not reach (0: PILEUP_BOUND; at most PILEUP_BOUND)
inline PileupPlan vs_pileup_plan_for(uint32_t n_nodes, uint32_t K, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound) {
    PileupPlan p = {};
    p.pending = pending;
    if (!bound) bound = PILEUP_BOUND;
    if (bound > PILEUP_BOUND || pending >= PILEUP_BOUND) {
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
    if (!n_ends || !n_nodes || !K || max_len < K) return p;  // no end holds an anchor: nothing pends either
    const bool fits = n_ends <= (PILEUP_BOUND - 1u) / (2ull * max_len);  // n_ends * 2 * max_len < 2^32, without forming a product that could wrap
    p.weight = fits ? n_ends * 2u * max_len : PILEUP_BOUND;
    if (!fits) {  // no fold can help inside one launch, whatever the bound asked for
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "%llu ends of up to %u bases could put 2^32 on one position: give the block in parts",
                 (unsigned long long)n_ends, max_len);
        return p;
    }
    p.fold_first = pending && pending + p.weight >= bound ? 1u : 0u;
    p.pending = (p.fold_first ? 0u : pending) + p.weight;
    // two workgroups of 1 024 threads per CU (22 KB of LDS each), as k_node_cover
    const uint64_t slots = (uint64_t)(n_cu ? n_cu : 1u) * 2u;
    uint64_t per = (n_ends + slots - 1u) / slots;
    if (per < PILEUP_MIN_ENDS) per = PILEUP_MIN_ENDS;
    if (per > PILEUP_MAX_ENDS) per = PILEUP_MAX_ENDS;
    p.ends_per_wg = per;
    p.grid = (uint32_t)((n_ends + per - 1u) / per);  // (at most 2^22: n_ends < 2^32, per >= 1 024)
    p.launch = 1u;
    return p;
}

#endif  // VS_PILEUP_PLAN_H
