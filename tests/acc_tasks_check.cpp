// Stand-alone host program over vstrains_amd/csrc/vs_acc_tasks.h (tests/test_pe_counter_tasks_cpu.py builds it with the host
// compiler and -fsanitize=address,undefined and reads what it prints).  No device, no HIP call.
//   for every (nl, nr) in 0..20 x 0..20: two lists of distinct nodes in random order, the pair's tasks written as
//   k_pe_accumulate writes them, every task entry decoded and walked as the kernel's lanes walk it (blocks of four list
//   words, the first stretch padded to whole blocks), and every counted cell printed:
//       P nl nr | left nodes | right nodes
//       C mat x y
//   then batch cuts over random task counts:
//       B cap n first last | task counts
// What the header promises about itself (task count, turns, partner counts, word round trip) is checked here and ends the
// program with a message and status 1; what the cells must be is the test's business (pe_counter_model.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../vstrains_amd/csrc/vs_acc_tasks.h"

#define LCAP 20u

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

static void fail(const char *what, uint32_t nl, uint32_t nr, uint32_t a) {
    fprintf(stderr, "acc_tasks_check: %s (nl %u, nr %u, a %u)\n", what, nl, nr, a);
    exit(1);
}

// a list of n distinct nodes below 200 in random order, in a buffer padded like the hand-off (whole quads + tail)
static std::vector<uint32_t> make_list(uint32_t n) {
    std::vector<uint32_t> pool(200), out(LCAP + 8u, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < 200u; i++) pool[i] = i;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t j = i + rnd(200u - i);
        const uint32_t t = pool[i]; pool[i] = pool[j]; pool[j] = t;
        out[i] = pool[i];
    }
    return out;
}

// One task entry as a lane of k_pe_accumulate takes it: decode, then blocks of four words from the partner list; a short
// row's x is the first word of either stretch.  Prints the cells; returns the turns the lane was busy for.
static uint32_t walk(uint32_t w, const std::vector<uint32_t> &l, const std::vector<uint32_t> &r, uint32_t nl, uint32_t nr, uint32_t *cells) {
    const uint32_t kind = vs_acc_entry_kind(w), a = vs_acc_entry_a(w);
    const VsAccSegs s = vs_acc_task_segs(kind, a, nl, nr);
    const uint32_t mat = kind != VS_ACC_NODE ? 1u : 0u, e = s.e;
    const std::vector<uint32_t> &plist = kind == VS_ACC_LEFT ? l : r;
    uint32_t x = kind == VS_ACC_NODE ? l[a] : 0u, p = s.p1, p2 = s.p2, busy = 0;
    bool fresh = true;
    for (uint32_t t = 0; t < 32u; t += 4u) {
        const uint32_t *ys = plist.data() + p;  // (the block's 16-byte load: p + 3 stays inside the padded buffer)
        if (p + 3u >= plist.size()) fail("a block load leaves the padded list", nl, nr, a);
        if (mat && fresh) x = ys[0];
        const uint32_t pb = p;
        p += 4u;
        fresh = p >= e;
        if (fresh) { p = p2; p2 = e; }
        for (uint32_t j = 0; j < 4u; j++) {
            if (pb + j >= e) continue;
            const uint32_t yv = ys[j];
            const uint32_t cx = (mat && yv < x) ? yv : x, cy = (mat && yv < x) ? x : yv;
            printf("C %u %u %u\n", mat, cx, cy);
            (*cells)++;
            busy = t + j + 1u;
        }
    }
    return busy;
}

int main() {
    for (uint32_t pair = 0; pair < 64u; pair++)
        for (uint32_t kind = 0; kind <= VS_ACC_RIGHT; kind++)
            for (uint32_t a = 0; a < LCAP; a++) {
                const uint32_t w = vs_acc_task_entry(pair, kind, a);
                if (!w || vs_acc_entry_pair(w) != pair || vs_acc_entry_kind(w) != kind || vs_acc_entry_a(w) != a) fail("entry round trip", pair, kind, a);
            }
    for (uint32_t nl = 0; nl <= LCAP; nl++)
        for (uint32_t nr = 0; nr <= LCAP; nr++) {
            const std::vector<uint32_t> l = make_list(nl), r = make_list(nr);
            printf("P %u %u |", nl, nr);
            for (uint32_t i = 0; i < nl; i++) printf(" %u", l[i]);
            printf(" |");
            for (uint32_t i = 0; i < nr; i++) printf(" %u", r[i]);
            printf("\n");
            // the tasks, in the order a lane writes them
            std::vector<uint32_t> words;
            if (nr)
                for (uint32_t a = 0; a < nl; a++) words.push_back(vs_acc_task_entry(37u, VS_ACC_NODE, a));
            for (uint32_t side = 0; side < 2u; side++) {
                const uint32_t n = side ? nr : nl, kind = side ? VS_ACC_RIGHT : VS_ACC_LEFT;
                if (n & 1u) words.push_back(vs_acc_task_entry(37u, kind, n >> 1));  // the middle row
                std::vector<uint32_t> seen(LCAP, 0u);
                for (uint32_t r = 0; r < 4u; r++) {  // the folded rows, class by class
                    const VsAccClass c = vs_acc_fold_class(n, r);
                    for (uint32_t i = 0; i < c.cnt; i++) {
                        const uint32_t a = c.a0 + 4u * i;
                        if (a >= n / 2u || seen[a]++) fail("a class names a row that is not a folded row, or one twice", nl, nr, a);
                        const VsAccSegs s = vs_acc_fold(n, a);
                        if (vs_acc_partners(s) != n + 1u) fail("partner count of a folded row", nl, nr, a);
                        if (vs_acc_turns(s) != c.turns) fail("a class's turns are not its rows'", nl, nr, a);
                        words.push_back(vs_acc_task_entry(37u, kind, a));
                    }
                }
                for (uint32_t a = 0; a < n / 2u; a++)
                    if (!seen[a]) fail("a folded row in no class", nl, nr, a);
                if ((n & 1u) && vs_acc_partners(vs_acc_fold(n, n >> 1)) != (n + 1u) / 2u) fail("partner count of the middle row", nl, nr, n >> 1);
            }
            if (words.size() != vs_acc_pair_tasks(nl, nr) || words.size() > 40u) fail("task count", nl, nr, 0);
            uint32_t cells = 0, partners = 0;
            for (uint32_t w : words) {
                const uint32_t kind = vs_acc_entry_kind(w), a = vs_acc_entry_a(w);
                if (!w || w > 0xFFFFu || vs_acc_entry_pair(w) != 37u || kind > VS_ACC_RIGHT) fail("task entry", nl, nr, a);
                const VsAccSegs s = vs_acc_task_segs(kind, a, nl, nr);
                const uint32_t turns = vs_acc_turns(s);
                if (turns == 0 || turns > 22u || turns < vs_acc_partners(s) || turns > vs_acc_partners(s) + 3u) fail("turns", nl, nr, a);
                if (s.p2 < s.e && ((s.e - s.p1 + 3u) & ~3u) - (s.e - s.p1) > ((s.e - s.p2 + 3u) & ~3u) - (s.e - s.p2)) fail("the row that pads more goes first", nl, nr, a);
                partners += vs_acc_partners(s);
                const uint32_t before = cells;
                if (walk(w, l, r, nl, nr, &cells) != turns) fail("the walk is not over after `turns` turns", nl, nr, a);
                if (cells - before != vs_acc_partners(s)) fail("the walk counts another number of cells than the task has partners", nl, nr, a);
            }
            if (partners != nl * nr + nl * (nl + 1u) / 2u + nr * (nr + 1u) / 2u) fail("partners of the pair", nl, nr, 0);
        }
    // batch cuts: rounds of n pairs with random list lengths, every region size a plan may name and a few others
    for (uint32_t rep = 0; rep < 400u; rep++) {
        const uint32_t n = rep % 7u == 0 ? 1u + rnd(64u) : 64u;
        const uint32_t top = rep % 3u == 0 ? 2u : LCAP;
        const uint32_t caps[] = {ACC_TASK_MIN, ACC_TASK_MIN + 1u, 64u, 100u, ACC_TASK_CAP - 1u, ACC_TASK_CAP};
        const uint32_t cap = caps[rep % 6u];
        std::vector<uint32_t> tasks(n);
        for (uint32_t i = 0; i < n; i++) tasks[i] = rep % 5u == 0 ? ACC_TASK_MIN : vs_acc_pair_tasks(rnd(top + 1u), rnd(top + 1u));
        for (uint32_t first = 0; first < n;) {
            const uint32_t last = vs_acc_batch_cut(tasks.data(), n, first, cap);
            printf("B %u %u %u %u |", cap, n, first, last);
            for (uint32_t i = 0; i < n; i++) printf(" %u", tasks[i]);
            printf("\n");
            if (last <= first || last > n) fail("a batch of no pairs", cap, n, first);
            first = last;
        }
    }
    return 0;
}
