// CPU checker of the library's owning buffer (vstrains_amd/csrc/vs_buf.h, product source, compiled unchanged): the template
// over an allocator that counts its live blocks and can be told to refuse the next allocation.  No device, no HIP call; the
// runtime's header is included for hipError_t only.  tests/test_buf_cpu.py asserts on what the scenarios report.
#include <stdint.h>
#include <stdlib.h>

#include <map>
#include <utility>

#include "../vstrains_amd/csrc/vs_buf.h"

namespace {
struct Counting {
    static std::map<void *, size_t> live;  // block -> bytes
    static int fail_next;                  // refuse this many allocations
    static bool poison_on_fail;            // write a wild value into the out-pointer of a refused allocation
    static uint64_t allocs, frees, bad_frees, peak_live;
    static size_t last_alloc;
    static void clear() {
        live.clear();
        fail_next = 0;
        poison_on_fail = false;
        allocs = frees = bad_frees = peak_live = 0;
        last_alloc = 0;
    }
    static hipError_t alloc(void **p, size_t bytes) {
        if (fail_next > 0) {
            fail_next--;
            if (poison_on_fail) *p = (void *)(uintptr_t)1;  // (else untouched, as the runtime leaves it)
            return hipErrorOutOfMemory;
        }
        *p = malloc(bytes ? bytes : 1);
        live[*p] = bytes;
        allocs++;
        last_alloc = bytes;
        if (live.size() > peak_live) peak_live = live.size();
        return hipSuccess;
    }
    static void free(void *p) {
        auto it = live.find(p);
        if (it == live.end()) {  // a double free, or a pointer this allocator never gave out
            bad_frees++;
            return;
        }
        live.erase(it);
        frees++;
        ::free(p);
    }
};
std::map<void *, size_t> Counting::live;
int Counting::fail_next = 0;
bool Counting::poison_on_fail = false;
uint64_t Counting::allocs = 0, Counting::frees = 0, Counting::bad_frees = 0, Counting::peak_live = 0;
size_t Counting::last_alloc = 0;

using Buf = VsBuf<Counting>;

// one observation of a buffer and the allocator: 8 words
uint64_t *note(uint64_t *o, const Buf &b, hipError_t e, bool fresh) {
    o[0] = b.ptr() != nullptr;
    o[1] = b.capacity();
    o[2] = e == hipSuccess ? 0 : e == hipErrorOutOfMemory ? 1 : 2;
    o[3] = fresh;
    o[4] = Counting::live.size();
    o[5] = Counting::peak_live;
    o[6] = Counting::last_alloc;
    o[7] = Counting::bad_frees;
    return o + 8;
}
}  // namespace

// Runs scenario `which`, writes observations of 8 words each to out (room for 16 of them); returns how many.
//   [0] pointer is not null  [1] capacity  [2] 0 ok / 1 out of memory / 2 another error  [3] "allocated anew"
//   [4] live blocks  [5] most live blocks at any time  [6] bytes of the last allocation  [7] frees of unknown pointers
extern "C" int vs_buf_check(int which, uint64_t *out) {
    Counting::clear();
    uint64_t *o = out;
    bool fresh = true;
    hipError_t e;
    switch (which) {
    case 0: {  // a refused reserve on an empty buffer, then a smaller one that succeeds
        Buf b;
        Counting::fail_next = 1;
        e = b.reserve(4000, 4000, &fresh);
        o = note(o, b, e, fresh);
        e = b.reserve(1000, 1000, &fresh);
        o = note(o, b, e, fresh);
        break;
    }
    case 1: {  // the same on a buffer that held memory: the slow_cap sequence
        Buf b;
        e = b.reserve(1000, 1000, &fresh);
        o = note(o, b, e, fresh);
        Counting::fail_next = 1;
        e = b.reserve(4000, 4000, &fresh);
        o = note(o, b, e, fresh);
        e = b.reserve(500, 500, &fresh);  // (below the capacity it had before the failure: must allocate all the same)
        o = note(o, b, e, fresh);
        break;
    }
    case 2: {  // an out-pointer the refused allocation wrote a wild value to, or left alone, does not survive
        Buf b;
        Counting::fail_next = 1;
        Counting::poison_on_fail = true;
        e = b.reserve(64, 64, &fresh);
        o = note(o, b, e, fresh);
        Buf c;
        e = c.reserve(64, 64, &fresh);
        o = note(o, c, e, fresh);
        Counting::fail_next = 1;
        Counting::poison_on_fail = false;
        e = c.reserve(128, 128, &fresh);
        o = note(o, c, e, fresh);
        break;
    }
    case 3: {  // below the capacity nothing happens; above it the old block goes first and the slack asked for is allocated
        Buf b;
        e = b.reserve(1000, 1500, &fresh);
        o = note(o, b, e, fresh);
        const void *p0 = b.ptr();
        e = b.reserve(1200, 5000, &fresh);
        o = note(o, b, e, fresh);
        o[-8] = b.ptr() == p0;  // (word 0 of this observation: the very same block)
        e = b.reserve(1500, 1500, &fresh);
        o = note(o, b, e, fresh);
        e = b.reserve(1501, 3000, &fresh);
        o = note(o, b, e, fresh);
        e = b.reserve(4000);  // (no slack given: exactly what is needed)
        o = note(o, b, e, false);
        break;
    }
    case 4: {  // move, release, take-over; every block freed exactly once when the objects die
        {
            Buf a, c;
            e = a.reserve(100, 100, &fresh);
            Buf b(std::move(a));
            o = note(o, a, e, fresh);  // the source of a move construction
            o = note(o, b, e, fresh);
            e = c.reserve(200, 200, &fresh);
            c = std::move(b);  // (c's own block goes)
            o = note(o, b, e, fresh);  // the source of a move assignment
            o = note(o, c, e, fresh);
            void *raw = c.release();
            o = note(o, c, e, fresh);  // after release: empty, and the block is still live
            Buf d;
            d.adopt(raw, 100);
            o = note(o, d, e, fresh);
            Buf f;
            e = f.reserve(300, 300, &fresh);
            o = note(o, f, e, fresh);
        }
        Buf none;
        o = note(o, none, hipSuccess, false);  // all objects gone
        o[-8 + 0] = Counting::allocs;
        o[-8 + 1] = Counting::frees;
        break;
    }
    default:
        return -1;
    }
    return (int)((o - out) / 8);
}
