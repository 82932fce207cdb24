// The reader of pe_info / st_info text (vstrains_amd/csrc/vs_info_read_core.h) as plain C++, for a host build under
// AddressSanitizer and UBSan (tests/test_info_read_cpu.py builds and runs this program).  The text, the name blob, the
// offsets, the name table and every window buffer lie in heap blocks of exactly their size, so a read in front of or behind
// any of them is found.  Every case is walked at the window that holds it whole and at every window from 16 to 64 bytes
// that its lines fit; the cells must be the same.  Prints "case <name> ..." per case, "walk ..." per sweep, then "OK".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../vstrains_amd/csrc/vs_info_read_core.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            failures++;                   \
        }                                 \
    } while (0)

struct Cell {
    uint32_t r, c;
    int64_t v;
    bool operator==(const Cell &o) const { return r == o.r && c == o.c && v == o.v; }
};
struct Result {
    int outcome = 0;  // 0 read, 1 flags, 2 malformed, 3 does not fit
    uint64_t bad_at = 0, lines = 0, skipped = 0, windows = 0;
    std::vector<Cell> cells;
};

struct Names {  // exactly sized heap blocks
    uint8_t *blob;
    uint64_t *off;
    IrSlot *table;
    IrNames nm;
    explicit Names(const std::vector<std::string> &names) {
        uint64_t total = 0;
        for (const auto &s : names) total += s.size();
        const uint32_t n = (uint32_t)names.size(), bits = ir_table_bits(n);
        blob = new uint8_t[total];
        off = new uint64_t[n + 1u];
        table = new IrSlot[(size_t)1u << bits];
        off[0] = 0;
        for (uint32_t i = 0; i < n; i++) {
            memcpy(blob + off[i], names[i].data(), names[i].size());
            off[i + 1u] = off[i] + names[i].size();
        }
        for (size_t s = 0; s < ((size_t)1u << bits); s++) table[s] = IrSlot{0u, IR_EMPTY};
        for (uint32_t i = 0; i < n; i++) CHECK(ir_table_insert(table, bits, blob, off, total, i), "insert %u", i);
        nm = IrNames{blob, off, table, total, n, bits};
    }
    ~Names() {
        delete[] blob;
        delete[] off;
        delete[] table;
    }
};

// the walk of vs_info_read_host, every window in a fresh block of exactly its bytes
static Result walk(const std::string &text_s, const IrNames &nm, uint32_t window) {
    Result res;
    const uint64_t size = text_s.size();
    uint8_t *text = new uint8_t[size];
    memcpy(text, text_s.data(), size);
    IrWalk w = ir_walk_begin(window);
    std::vector<uint8_t> carry;
    uint32_t flags = 0;
    bool bad = false;
    for (uint64_t at = 0; at < size;) {
        const uint32_t room = ir_walk_room(w);
        if (!room) {
            res.outcome = 3;
            delete[] text;
            return res;
        }
        const uint32_t fresh = (uint32_t)(size - at < room ? size - at : room), total = w.carry + fresh;
        uint8_t *buf = new uint8_t[total];
        if (w.carry) memcpy(buf, carry.data(), w.carry);
        memcpy(buf + w.carry, text + at, fresh);
        at += fresh;
        res.windows++;
        const IrScan scan = ir_scan_host(buf, total);
        flags |= scan.flags;
        const uint32_t limit = ir_walk_limit(w, scan, total, at == size);
        const IrHostReader rd = {buf, total};
        bool malformed = false;
        for (uint32_t p = 0; p < limit;) {
            const uint32_t stop = ir_line_stop(rd, p, total);
            Cell c = {0, 0, 0};
            const int what = ir_parse_line(nm, rd, p, stop, &c.r, &c.c, &c.v);
            if (what == IR_MALFORMED) {
                malformed = bad = true;
                res.bad_at = w.base + p;
                break;
            }
            res.lines++;
            if (what == IR_SKIPPED) res.skipped++;
            else res.cells.push_back(c);
            p = stop + 1u;
        }
        ir_walk_next(w, scan, total, malformed);
        carry.assign(buf + (total - w.carry), buf + total);
        delete[] buf;
    }
    delete[] text;
    res.outcome = flags ? 1 : bad ? 2 : 0;
    return res;
}

static bool fits(const std::string &text, uint32_t window, int outcome, uint64_t bad_at) {
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at);
        const size_t len = nl == std::string::npos ? text.size() - at : nl + 1u - at;
        if (len == 1u && nl != std::string::npos) return true;
        if (len > window) return false;
        if (outcome == 2 && at == bad_at) return true;
        at += len;
    }
    return true;
}

static void run_case(const char *name, const std::vector<std::string> &names, const std::string &text, int outcome, const std::vector<Cell> &cells,
                     uint64_t skipped, uint64_t bad_at) {
    Names N(names);
    const Result whole = walk(text, N.nm, (uint32_t)(text.size() > 16u ? text.size() : 16u));
    CHECK(whole.outcome == outcome, "%s: outcome %d, expected %d", name, whole.outcome, outcome);
    if (outcome == 0) CHECK(whole.cells == cells && whole.skipped == skipped, "%s: %zu cells, %llu skipped", name, whole.cells.size(), (unsigned long long)whole.skipped);
    if (outcome == 2) CHECK(whole.bad_at == bad_at, "%s: malformed at %llu, expected %llu", name, (unsigned long long)whole.bad_at, (unsigned long long)bad_at);
    printf("case %s outcome=%d cells=%zu\n", name, whole.outcome, whole.cells.size());
    unsigned swept = 0;
    for (uint32_t window = 16; window <= 64; window++) {
        const Result r = walk(text, N.nm, window);
        if (!fits(text, window, outcome, bad_at)) {
            CHECK(r.outcome == 3, "%s: window %u: outcome %d where a line does not fit", name, window, r.outcome);
            continue;
        }
        swept++;
        CHECK(r.outcome == outcome, "%s: window %u: outcome %d", name, window, r.outcome);
        if (outcome == 0) CHECK(r.cells == whole.cells && r.skipped == whole.skipped && r.lines == whole.lines, "%s: window %u: cells differ", name, window);
        if (outcome == 2) CHECK(r.bad_at == bad_at, "%s: window %u: malformed at %llu", name, window, (unsigned long long)r.bad_at);
    }
    printf("walk %s windows=%u\n", name, swept);
}

int main() {
    const std::vector<std::string> abc = {"1", "2", "3"};
    const int64_t max64 = 9223372036854775807ll, min64 = -max64 - 1;
    run_case("empty", abc, "", 0, {}, 0, 0);
    run_case("newline_alone", abc, "\n", 0, {}, 0, 0);
    run_case("no_final_newline", {"7&8*0", "9"}, "7&8*0:9:57", 0, {{0, 1, 5}}, 0, 0);
    run_case("one_character", abc, "1:2:3\nx", 2, {}, 0, 6);
    run_case("empty_line", abc, "1:2:3\n\nnot a line\n1:2:4\n", 0, {{0, 1, 3}}, 0, 0);
    run_case("fields", abc, "1:2:3:4\n1:3:5:x:y\n2:3:6:\n", 0, {{0, 1, 3}, {0, 2, 5}, {1, 2, 6}}, 0, 0);
    run_case("signs", abc, "1:2:+5\n2:3:-5\n", 0, {{0, 1, 5}, {1, 2, -5}}, 0, 0);
    run_case("extremes", abc, "1:2:9223372036854775807\n1:3:-9223372036854775808\n", 0, {{0, 1, max64}, {0, 2, min64}}, 0, 0);
    run_case("beyond_max", abc, "1:2:1\n1:2:9223372036854775808\n", 2, {}, 0, 6);
    run_case("beyond_min", abc, "1:2:-9223372036854775809\n", 2, {}, 0, 0);
    run_case("unknown_good", abc, "1:9:5\n9:1:5\n1:2:1\n", 0, {{0, 1, 1}}, 2, 0);
    run_case("unknown_bad", abc, "1:2:1\n1:9:x\n", 2, {}, 0, 6);
    run_case("listed_twice", {"1", "2", "1"}, "1:2:3\n", 0, {{2, 1, 3}}, 0, 0);
    run_case("prefixes", {"1", "12", "1&2*0"}, "1:12:1\n12:1&2*0:2\n1&2*0:1:3\n1&2:1:4\n", 0, {{0, 1, 1}, {1, 2, 2}, {2, 0, 3}}, 1, 0);
    run_case("empty_id", abc, ":1:5\n1::5\n1:2:1\n", 0, {{0, 1, 1}}, 2, 0);
    run_case("two_malformed", abc, "1:2:3\n1:2\n1:2:x\n", 2, {}, 0, 6);
    run_case("long_malformed", abc, "1:2:" + std::string(70, '9') + "\n", 2, {}, 0, 0);
    run_case("carriage_return", abc, "1:2:3\r\n", 1, {}, 0, 0);
    run_case("high_byte", abc, "1:2:3\n1:\x80:4\n", 1, {}, 0, 0);
    run_case("cr_behind_the_end", abc, "1:2:3\n\n1:2:4\r\n", 1, {}, 0, 0);
    run_case("same_hash", {"17", "26"}, "17:26:1\n0V:26:2\n26:0V:3\n", 0, {{0, 1, 1}}, 2, 0);  // "0V" has the hash of "17"
    {  // no name at all: a table of two free slots, an empty blob
        run_case("no_names", {}, "1:2:3\n", 0, {}, 1, 0);
    }
    {  // many equal lines: a cut on every position of a line
        std::string text;
        std::vector<Cell> cells;
        for (int i = 0; i < 40; i++) text += "12:345:67890\n", cells.push_back({0, 1, 67890});
        run_case("equal_lines", {"12", "345"}, text, 0, cells, 0, 0);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
