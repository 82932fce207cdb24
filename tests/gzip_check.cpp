// The parallel gzip decoder (vstrains_amd/csrc/vs_gzip_core.h) as plain C++ with one lane, for a host build under
// AddressSanitizer and UBSan (tests/test_gzip_device_cpu.py builds and runs this program).  Usage:
//     gzip_check DIR small NAME...
// DIR/NAME.gz is a case, DIR/NAME.txt its text when it is a good one.  Every stream lies in a heap buffer of exactly its
// size (the decoder's own symbol, member and text buffers are exactly sized too), and goes through the whole path at three
// granularities.  zlib, linked in, is the oracle: a good case must give its text, a case without text must be refused, and
// the stream `small` is also run cut at every byte length and with every single bit of its first 64 bytes flipped -- no
// call may return OK with a text other than the one zlib makes of the same bytes.  Prints "<name> good|refused ...", the
// two tallies, then "OK".
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../vstrains_amd/csrc/vs_gzip_core.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            failures++;                   \
        }                                 \
    } while (0)

static bool read_file(const std::string &path, std::vector<uint8_t> &v) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    v.clear();
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

// what zlib makes of a whole file of gzip members: true and the text, or false
static bool zlib_text(const std::vector<uint8_t> &data, std::vector<uint8_t> &text) {
    text.clear();
    size_t at = 0;
    if (data.empty()) return true;
    std::vector<uint8_t> buf(1 << 16);
    while (at < data.size()) {
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, 31) != Z_OK) return false;
        z.next_in = const_cast<Bytef *>(data.data() + at);
        z.avail_in = (uInt)(data.size() - at);
        int rc = Z_OK;
        while (rc == Z_OK) {
            z.next_out = buf.data();
            z.avail_out = (uInt)buf.size();
            rc = inflate(&z, Z_NO_FLUSH);
            text.insert(text.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
            if (rc == Z_BUF_ERROR) break;  // (no progress: the input ended inside the member)
        }
        at = data.size() - z.avail_in;
        inflateEnd(&z);
        if (rc != Z_STREAM_END) return false;
    }
    return true;
}

// one call on an exactly sized copy
static uint32_t ours(const std::vector<uint8_t> &data, uint32_t gran, std::vector<uint8_t> &text, GzInfo &info) {
    uint8_t *p = new uint8_t[data.size() ? data.size() : 1];
    if (!data.empty()) memcpy(p, data.data(), data.size());
    gz_inflate_one_lane(data.empty() ? nullptr : p, data.size(), gran, text, info);
    delete[] p;
    return (uint32_t)info.status;
}

static const uint32_t GRANS[3] = {0u, 64u, 4096u};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    for (int a = 3; a < argc; a++) {
        const std::string name = argv[a];
        std::vector<uint8_t> data, want, got;
        CHECK(read_file(dir + "/" + name + ".gz", data), "%s: no file", name.c_str());
        const bool good = read_file(dir + "/" + name + ".txt", want);
        std::vector<uint8_t> ztext;
        CHECK(zlib_text(data, ztext) == good && (!good || ztext == want), "%s: zlib's verdict is not the case's", name.c_str());
        GzInfo info;
        for (uint32_t gran : GRANS) {
            const uint32_t st = ours(data, gran, got, info);
            if (good) CHECK(st == INF_OK && got == want, "%s: gran %u status %u, %zu bytes of %zu", name.c_str(), gran, st, got.size(), want.size());
            else CHECK(st != INF_OK && got.empty(), "%s: gran %u accepted", name.c_str(), gran);
        }
        printf("%s %s status=%u runs=%llu dropped=%llu members=%llu\n", name.c_str(), good ? "good" : "refused", (unsigned)info.status,
               (unsigned long long)info.chain_runs, (unsigned long long)info.dropped, (unsigned long long)info.members);
    }
    // the small stream, cut and flipped
    const std::string name = argv[2];
    std::vector<uint8_t> data, want, got, ztext;
    CHECK(read_file(dir + "/" + name + ".gz", data) && read_file(dir + "/" + name + ".txt", want), "%s: no files", name.c_str());
    GzInfo info;
    CHECK(ours(data, 0, got, info) == INF_OK && got == want && info.members == 2 && info.chain_runs >= 4, "%s: status %u", name.c_str(),
          (unsigned)info.status);
    unsigned calls = 0, ok = 0;
    for (size_t cut = 0; cut < data.size(); cut++) {
        const std::vector<uint8_t> part(data.begin(), data.begin() + cut);
        const bool zok = zlib_text(part, ztext) && cut > 0;
        for (uint32_t gran : GRANS) {
            const uint32_t st = ours(part, gran, got, info);
            calls++;
            if (st == INF_OK) {
                ok++;
                CHECK(zok && got == ztext, "%s cut at %zu, gran %u: OK with a text that is not zlib's", name.c_str(), cut, gran);
            }
        }
    }
    printf("%s cuts %u ok %u\n", name.c_str(), calls, ok);
    CHECK(ok == 3u, "%s: %u cuts accepted (the cut between the members, at three granularities, is the one whole file)", name.c_str(), ok);
    calls = ok = 0;
    for (size_t bit = 0; bit < 512 && bit < data.size() * 8; bit++) {
        std::vector<uint8_t> flipped(data);
        flipped[bit >> 3] ^= (uint8_t)(1u << (bit & 7u));
        const bool zok = zlib_text(flipped, ztext);
        for (uint32_t gran : {0u, 4096u}) {
            const uint32_t st = ours(flipped, gran, got, info);
            calls++;
            if (st == INF_OK) {
                ok++;
                CHECK(zok && got == ztext, "%s bit %zu, gran %u: OK with a text that is not zlib's", name.c_str(), bit, gran);
            }
        }
    }
    printf("%s flips %u ok %u\n", name.c_str(), calls, ok);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
