// cybervision_amd/csrc/png_decode_common.hpp on the CPU, built with AddressSanitizer and UBSan by tests/test_png_in_host_cpu.py:
//   png_in_host parse FILE            one line of JSON: the return code and, when it is 0, what the parser found
//   png_in_host fuzz FILE SEED FLIPS  the parser over every truncation of the file and over FLIPS seeded corruptions of
//                                     it; prints how often each code came back
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

// the parser on an exact-size copy (a read past the file's end is a read past the allocation); what it accepts must lie in the file
static int run(const std::vector<uint8_t> &data, pd::Header &h)
{
    std::vector<uint8_t> exact(data.begin(), data.end());
    const int rc = pd::parse(exact.data(), exact.size(), h);
    if (rc != pd::OK) return rc;
    if (h.idat.empty() || h.width == 0 || h.height == 0 || h.bpp == 0 || h.row_bytes == 0) std::abort();
    uint64_t bytes = 0;
    for (const pd::Idat &c : h.idat) {
        if (c.offset + c.length + 4 > exact.size()) std::abort();
        bytes += c.length;
    }
    if (bytes != h.idat_bytes || h.palette_entries > 256 || (h.colour == 3 && h.palette_entries == 0)) std::abort();
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> data = read_file(argv[2]);
    if (mode == "parse") {
        pd::Header h;
        const int rc = run(data, h);
        if (rc != pd::OK) {
            std::printf("{\"code\": %d}\n", rc);
            return 0;
        }
        std::printf("{\"code\": 0, \"width\": %u, \"height\": %u, \"colour\": %u, \"depth\": %u, \"interlace\": %u, \"channels\": %u, \"bpp\": %u, "
                    "\"row_bytes\": %llu, \"focal\": %u, \"flags\": %u, \"palette\": [",
                    h.width, h.height, h.colour, h.depth, h.interlace, h.channels, h.bpp, (unsigned long long)h.row_bytes, h.focal_length_35mm, h.flags);
        for (uint32_t k = 0; k < 3 * h.palette_entries; k++) std::printf("%s%u", k ? ", " : "", h.palette[k]);
        std::printf("], \"idat\": [");
        for (size_t k = 0; k < h.idat.size(); k++)
            std::printf("%s[%llu, %u, %u]", k ? ", " : "", (unsigned long long)h.idat[k].offset, h.idat[k].length, h.idat[k].crc);
        std::printf("]}\n");
        return 0;
    }
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
