// The work units of k_pe_accumulate (vs_pe.hip, K4): a pair of end lists as TASKS, one per matrix row.  Plain C++ and pure:
// a host compiler takes this header as it is (tests/acc_tasks_check.cpp, tests/test_pe_counter_tasks_cpu.py), hipcc takes it
// for the kernel, which packs, folds, counts and cuts with these functions and no others.
//
// A pair with a left list l (nl nodes) and a right list r (nr nodes) adds (PE_Inference.py:174-188)
//   node_mat [l[a]][r[b]]                          for every a < nl, b < nr
//   short_mat[min][max] of (e[a], e[b]), a <= b    for either end's list e
// and becomes
//   nl node rows          (VS_ACC_NODE, a): x = l[a] against the whole right list, nr partners        (none when nr = 0)
//   ceil(nl / 2) left and ceil(nr / 2) right short rows (VS_ACC_LEFT / VS_ACC_RIGHT, a), a < ceil(n / 2): row a of the
//       triangle -- x = e[a] against positions [a, n) -- FOLDED with its mirror row n-1-a -- x = e[n-1-a] against
//       [n-1-a, n): n + 1 partners whatever a is.  The middle row of an odd n (a = n-1-a) stands alone, (n + 1) / 2 partners.
// 20 + 10 + 10 = 40 tasks at most.
//
// A lane walks a task's partners in BLOCKS of four list words (one 16-byte load at the word the block starts at), so a
// row begins at a block boundary.  The two rows of a folded task are therefore walked one after the other with the first
// padded to whole blocks, and the row that wastes fewer padding turns goes first: `turns` = pad4(first) + second is what a
// task costs a lane, at most 22, and what the tasks of a batch are ordered by.
#ifndef VS_ACC_TASKS_H
#define VS_ACC_TASKS_H
#include <stdint.h>

#include "vs_pe_plan.h"

#define VS_ACC_NODE 0u
#define VS_ACC_LEFT 1u
#define VS_ACC_RIGHT 2u

// tasks of a pair
VS_PLAN_FN uint32_t vs_acc_pair_tasks(uint32_t nl, uint32_t nr) { return (nr ? nl : 0u) + ((nl + 1u) >> 1) + ((nr + 1u) >> 1); }

// The partner positions of a task in its partner list (the right list for a node row, the end's own list for a short
// row): [p1, e), then [p2, e); p2 == e: no second stretch.  Both rows of a fold end at the list's end.
struct VsAccSegs {
    uint32_t p1, p2, e;
};
VS_PLAN_FN VsAccSegs vs_acc_fold(uint32_t n, uint32_t a) {  // short row a < ceil(n / 2) of an n-list
    const uint32_t a2 = n - 1u - a;
    if (a2 == a) return VsAccSegs{a, n, n};
    // row a has n - a partners, row a2 has a + 1: first the one that pads fewer turns up to a whole block
    const bool a_first = ((0u - (n - a)) & 3u) <= ((0u - (a + 1u)) & 3u);
    return VsAccSegs{a_first ? a : a2, a_first ? a2 : a, n};
}
VS_PLAN_FN VsAccSegs vs_acc_task_segs(uint32_t kind, uint32_t a, uint32_t nl, uint32_t nr) {
    return kind == VS_ACC_NODE ? VsAccSegs{0u, nr, nr} : vs_acc_fold(kind == VS_ACC_LEFT ? nl : nr, a);
}
// turns a lane spends on the task
VS_PLAN_FN uint32_t vs_acc_turns(const VsAccSegs &s) {
    return s.p2 < s.e ? ((s.e - s.p1 + 3u) & ~3u) + (s.e - s.p2) : s.e - s.p1;
}
// partners of the task
VS_PLAN_FN uint32_t vs_acc_partners(const VsAccSegs &s) { return (s.e - s.p1) + (s.e - s.p2); }

// The tasks of a batch are ordered by their turns, so a lane must know how many tasks of which length its pair brings
// before it writes them.  Node rows: nl of nr turns.  The middle row of an odd list: (n + 1) / 2.  The folded rows of an
// n-list, a < n / 2, fall into four CLASSES by r = (n - a) & 3, the partners of row a beyond whole blocks: a class is the
// rows a0, a0 + 4, ... (cnt of them), and all of them take the same turns, n + 1 + the padding of the row that goes first.
struct VsAccClass {
    uint32_t a0, cnt, turns;
};
VS_PLAN_FN VsAccClass vs_acc_fold_class(uint32_t n, uint32_t r) {
    const uint32_t a0 = (n - r) & 3u;
    const uint32_t pad_a = (0u - r) & 3u, pad_m = (r - n - 1u) & 3u;  // row a first / its mirror row (a + 1 partners) first
    return VsAccClass{a0, ((n >> 1) + 3u - a0) >> 2, n + 1u + (pad_a <= pad_m ? pad_a : pad_m)};
}

// The task entry, 16 bits: pair in the wavefront's round (6 bits) | kind (2) | a (5) | 0x8000.  0 = no task.  (What a task
// costs follows from the entry and the pair's list lengths -- vs_acc_task_segs, vs_acc_turns -- so it is not stored: two
// entries per LDS word let a round of 64 pairs be one batch nearly always.)
VS_PLAN_FN uint16_t vs_acc_task_entry(uint32_t pair, uint32_t kind, uint32_t a) { return (uint16_t)(0x8000u | pair | kind << 6 | a << 8); }
VS_PLAN_FN uint32_t vs_acc_entry_pair(uint32_t w) { return w & 63u; }
VS_PLAN_FN uint32_t vs_acc_entry_kind(uint32_t w) { return (w >> 6) & 3u; }
VS_PLAN_FN uint32_t vs_acc_entry_a(uint32_t w) { return (w >> 8) & 31u; }

// The batch cut: a wavefront holds the task counts of its n pairs (n <= 64) and takes, from pair `first` on, the longest
// run whose tasks fit `cap` entries, at least one pair (cap >= ACC_TASK_MIN, so one pair always fits).  -> the first pair
// of the next batch.  `fits` is the test the kernel applies to the inclusive prefix sums of a wavefront scan.
VS_PLAN_FN bool vs_acc_batch_fits(uint32_t tasks_incl, uint32_t cap) { return tasks_incl <= cap; }
inline uint32_t vs_acc_batch_cut(const uint32_t *tasks, uint32_t n, uint32_t first, uint32_t cap) {
    uint32_t incl = 0, last = first;
    while (last < n && vs_acc_batch_fits(incl + tasks[last], cap)) incl += tasks[last++];
    return last;
}

#endif  // VS_ACC_TASKS_H
