// cybervision_amd/csrc/png_decode_common.hpp with adam7 = true on the CPU, built with AddressSanitizer and UBSan by
// tests/test_png_adam7_host_cpu.py:
//   png_adam7_host parse FILE ...        per file one line of JSON: the return code and, when it is 0, the header, the pass
//                                        table and `filtered`; "plain" is the code parse(.., false) gives the same bytes
//   png_adam7_host fuzz FILE SEED FLIPS  the parser over every truncation of the file and over FLIPS seeded corruptions of
//                                        it; prints how often each code came back
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/png_decode_common.hpp"

namespace pd = png_decode_common;

static std::vector<uint8_t> read_file(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// the parser on an exact-size copy (a read past the file's end is a read past the allocation); what it accepts must hold together
static int run(const std::vector<uint8_t> &data, pd::Header &h, bool adam7 = true)
{
    std::vector<uint8_t> exact(data.begin(), data.end());
    const int rc = pd::parse(exact.data(), exact.size(), h, adam7);
    if (rc != pd::OK) return rc;
    if (h.idat.empty() || h.width == 0 || h.height == 0 || h.bpp == 0 || h.row_bytes == 0) std::abort();
    for (const pd::Idat &c : h.idat)
        if (c.offset + c.length + 4 > exact.size()) std::abort();
    if (h.interlace > 1 || (h.interlace && !adam7) || h.pass_entries != (h.interlace ? 7u : 1u)) std::abort();
    uint64_t bytes = 0, rows = 0, pixels = 0;
    uint32_t passes = 0;
    for (uint32_t p = 0; p < h.pass_entries; p++) {
        const pd::Pass &e = h.pass[p];
        if (e.first_row != rows || e.offset != bytes) std::abort();
        if ((e.width == 0) != (e.height == 0) || (e.width == 0) != (e.row_bytes == 0)) std::abort();
        bytes += (e.row_bytes + 1) * e.height, rows += e.height, pixels += (uint64_t)e.width * e.height, passes += e.height != 0;
    }
    if (bytes != h.filtered || bytes >= pd::MAX_FILTERED || rows != h.pass_rows || passes != h.passes || h.pass[0].height == 0) std::abort();
    if (pixels != (uint64_t)h.width * h.height) std::abort(); // every pixel is in one pass
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    for (int file = 2; mode == "parse" && file < argc; file++) {
        const std::vector<uint8_t> data = read_file(argv[file]);
        pd::Header h, plain;
        const int rc = run(data, h), rc_plain = run(data, plain, false);
        if (rc != pd::OK) {
            std::printf("{\"code\": %d, \"plain\": %d}\n", rc, rc_plain);
            continue;
        }
        std::printf("{\"code\": 0, \"plain\": %d, \"width\": %u, \"height\": %u, \"colour\": %u, \"depth\": %u, \"interlace\": %u, \"channels\": %u, \"bpp\": %u, "
                    "\"focal\": %u, \"flags\": %u, \"palette_entries\": %u, \"idat\": %zu, \"passes\": %u, \"pass_rows\": %u, \"filtered\": %llu, \"pass_table\": [",
                    rc_plain, h.width, h.height, h.colour, h.depth, h.interlace, h.channels, h.bpp, h.focal_length_35mm, h.flags, h.palette_entries,
                    h.idat.size(), h.passes, h.pass_rows, (unsigned long long)h.filtered);
        for (uint32_t p = 0; p < h.pass_entries; p++) {
            const pd::Pass &e = h.pass[p];
            std::printf("%s[%u, %u, %llu, %u, %llu, %u, %u, %u, %u]", p ? ", " : "", e.width, e.height, (unsigned long long)e.row_bytes, e.first_row,
                        (unsigned long long)e.offset, e.x0, e.y0, e.log_dx, e.log_dy);
        }
        std::printf("]}\n");
    }
    if (mode == "parse") return 0;
    const std::vector<uint8_t> data = read_file(argv[2]);
    if (mode == "fuzz" && argc >= 5) {
        unsigned long long state = std::strtoull(argv[3], nullptr, 10) * 2654435761ull + 1;
        const int flips = std::atoi(argv[4]);
        auto next = [&]() { // (a 64-bit LCG: the corruptions are the same on every run)
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            return (uint32_t)(state >> 33);
        };
        int counts[3] = {0, 0, 0};
        auto tally = [&](const std::vector<uint8_t> &bytes) {
            pd::Header h;
            const int rc = run(bytes, h);
            if (rc != pd::OK && rc != pd::INVALID && rc != pd::UNSUPPORTED) std::abort();
            counts[rc == pd::OK ? 0 : rc == pd::INVALID ? 1 : 2]++;
        };
        for (size_t cut = 0; cut < data.size(); cut++) tally(std::vector<uint8_t>(data.begin(), data.begin() + (long)cut));
        for (int f = 0; f < flips && !data.empty(); f++) {
            std::vector<uint8_t> bytes = data;
            const uint32_t changes = 1 + next() % 3;
            for (uint32_t k = 0; k < changes; k++) {
                const size_t at = next() % bytes.size();
                const uint32_t kind = next() % 3;
                bytes[at] = kind == 0 ? (uint8_t)(bytes[at] ^ (1u << (next() % 8))) : kind == 1 ? (uint8_t)next() : 0xFF;
            }
            tally(bytes);
        }
        std::printf("%d %d %d\n", counts[0], counts[1], counts[2]);
        return 0;
    }
    return 2;
}
