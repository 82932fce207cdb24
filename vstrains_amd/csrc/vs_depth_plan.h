// The launch plan of one depth pass (vs_node_depth): every decision taken before k_node_depth (vs_pe.hip) is launched --
// route, workgroups, ends per workgroup, LDS -- as ONE pure function of scalars, in the style of vs_pe_plan.h.  Plain C++:
// a host compiler takes this header as it is, hipcc takes it for the kernel, which reads its LDS layout from here.
//
// What the pass computes.  With K = k + 1, KC[n] is the number of triples (read end e, read offset i, table entry of
// node n) such that end_e[i : i + K] is a key of the reference's (k+1)-mer table (PE_Inference.py:117-135,
// oracle/pe_oracle.py:build_table) that holds that entry: the sum over all read ends of the `v` the mapping kernels
// compute per (end, node) BEFORE the acceptance test.  Every end of a block counts, whatever its mate is like.
#ifndef VS_DEPTH_PLAN_H
#define VS_DEPTH_PLAN_H
#include <stdint.h>
#include <stdio.h>

#include "../../include/vstrains_hip.h"

#define DEPTH_TPB 1024u         // threads of a k_node_depth workgroup: sixteen wavefronts, each working through batches of 64 ends
#define DEPTH_WAVES (DEPTH_TPB / 64u)
#define DEPTH_LDS_WORDS 40960u  // 160 KB: what one workgroup may take of a CU's LDS
// LDS words of one wavefront: the scan of its 64 ends' probe counts [65], the scan of 64 probes' posting counts [65], the
// probes' payloads and (end, read offset) [3 x 64], the combining slots of the global route, node and sum [2 x 64]
#define DEPTH_WAVE_WORDS 464u
#define DEPTH_HEAD_WORDS 4u     // the workgroup's batch counter (and three words of alignment)
// nodes whose dense uint32 counters fit beside that: 33 532
#define DEPTH_LDS_NODES (DEPTH_LDS_WORDS - DEPTH_HEAD_WORDS - DEPTH_WAVES * DEPTH_WAVE_WORDS)
#define DEPTH_MIN_ENDS (64u * DEPTH_WAVES)  // a workgroup's share is at least one batch per wavefront
#define DEPTH_MAX_ENDS (1u << 31)           // ... and its batch counter (32 bits, sixteen wavefronts overshoot by 64 each) cannot wrap

enum { VS_DEPTH_NONE = 0, VS_DEPTH_LDS = 1, VS_DEPTH_GLOBAL = 2 };

struct DepthPlan {
    int status;  // VS_OK, or VS_E_RANGE with msg
    char msg[128];
    uint32_t route;        // VS_DEPTH_NONE: nothing is launched (no ends, or no end holds a window)
    uint32_t grid;         // workgroups
    uint64_t ends_per_wg;  // workgroup g takes ends [g * ends_per_wg, (g + 1) * ends_per_wg)
    uint64_t wrap_ends;    // the most ends a workgroup's LDS counters allow (ends * (max_len - K + 1) < 2^32)
    uint32_t lds_nodes;    // dense counters in LDS (0 on the global route)
    uint64_t lds_bytes;
};

inline uint64_t vs_depth_lds_words(uint32_t lds_nodes) {
    return (((uint64_t)lds_nodes + 3u) & ~3ull) + DEPTH_HEAD_WORDS + (uint64_t)DEPTH_WAVES * DEPTH_WAVE_WORDS;
}

// n_nodes, K: the index; n_ends, max_len: the block; n_cu: compute units of the device
inline DepthPlan vs_depth_plan_for(uint32_t n_nodes, uint32_t K, uint64_t n_ends, uint32_t max_len, uint32_t n_cu) {
    DepthPlan p = {};
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
    if (!n_ends || !n_nodes || !K || max_len < K) return p;  // no end holds a (k+1)-window
    const bool dense = n_nodes <= DEPTH_LDS_NODES;
    p.route = dense ? VS_DEPTH_LDS : VS_DEPTH_GLOBAL;
    p.lds_nodes = dense ? n_nodes : 0u;
    p.lds_bytes = sizeof(uint32_t) * vs_depth_lds_words(p.lds_nodes);
    // An LDS counter takes len - K + 1 per match; the windows of an end are max_len - K + 1 at most, so a workgroup of
    // `ends` ends stays below 2^32 per node while ends * (max_len - K + 1) < 2^32.  (A (k+1)-mer that repeats inside one
    // node is counted at each of its positions and can exceed that; the kernel carries such a wrap into the 64-bit total,
    // so the bound keeps the carry rare instead of keeping the sum right.)
    const uint64_t span = (uint64_t)max_len - K + 1u;
    p.wrap_ends = 0xFFFFFFFFull / span;  // the largest count with ends * span <= 2^32 - 1
    uint64_t cap = p.wrap_ends < DEPTH_MAX_ENDS ? p.wrap_ends : DEPTH_MAX_ENDS;
    if (cap < 1u) cap = 1u;
    // as many workgroups as the device holds at once -- two of 1 024 threads per CU where their LDS allows, else one: every
    // workgroup ends with one pass over its counters, and more workgroups mean more atomics on the same totals
    const uint32_t per_cu = 2ull * p.lds_bytes <= sizeof(uint32_t) * (uint64_t)DEPTH_LDS_WORDS ? 2u : 1u;
    const uint64_t slots = (uint64_t)(n_cu ? n_cu : 1u) * per_cu;
    uint64_t per = (n_ends + slots - 1u) / slots;
    if (per < DEPTH_MIN_ENDS) per = DEPTH_MIN_ENDS;
    if (per > cap) per = cap;
    p.ends_per_wg = per;
    const uint64_t grid = (n_ends + per - 1u) / per;
    if (grid > 0x7FFFFFFFull) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "%llu ends of up to %u bases need more workgroups than one launch takes", (unsigned long long)n_ends, max_len);
        p.route = VS_DEPTH_NONE;
        return p;
    }
    p.grid = (uint32_t)grid;
    return p;
}

#endif  // VS_DEPTH_PLAN_H
