// cybervision_amd/csrc/tiff_common.hpp's extended walk (parse(.., extended = true)) on the CPU, built with
// AddressSanitizer and UBSan by tests/test_tiff_ext_host_cpu.py:
//   tiff_ext_host parse FILE            one line of JSON: the return code and, when it is 0, the frame, the tile geometry and the stream table
//   tiff_ext_host fuzz FILE SEED FLIPS  the walk over every truncation of the file and over FLIPS seeded corruptions of it;
//                                       prints how often each code came back
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/tiff_common.hpp"

namespace tc = tiff_common;

static std::vector<uint8_t> read_file(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

static uint32_t f32_bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// the walk on an exact-size copy (a read past the file's end is a read past the allocation); what it accepts must lie in the
// file, and the streams must cover the image
static int run(const std::vector<uint8_t> &data, tc::Header &h)
{
    std::vector<uint8_t> exact(data.begin(), data.end());
    const int rc = tc::parse(exact.data(), exact.size(), h, true);
    if (rc != tc::OK) return rc;
    if (h.strips.empty() || h.width == 0 || h.height == 0) std::abort();
    const bool tiled = h.tile_width != 0;
    if (tiled && (h.tile_width % 16 || h.tile_length % 16 || (uint64_t)h.tiles_across * h.tiles_down != h.strips.size())) std::abort();
    if (tiled && ((uint64_t)h.tiles_across * h.tile_width < h.width || (uint64_t)h.tiles_down * h.tile_length < h.height)) std::abort();
    uint64_t rows = 0;
    for (const tc::Strip &s : h.strips) {
        if ((uint64_t)s.offset + s.count > exact.size() || s.rows == 0 || s.row_bytes == 0) std::abort();
        if (h.compression == tc::COMPRESSION_NONE && s.count < (uint64_t)s.rows * s.row_bytes) std::abort();
        if (tiled && s.row_bytes != (uint64_t)h.tile_width * h.samples * (h.bits / 8)) std::abort(); // (nothing wrapped)
        if (s.x >= h.width || s.y >= h.height || (uint64_t)s.rows * s.row_bytes >= (1ull << 31)) std::abort();
        rows += s.rows;
    }
    if (!tiled && rows != h.height) std::abort();
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> data = read_file(argv[2]);
    if (mode == "parse") {
        tc::Header h;
        const int rc = run(data, h);
        if (rc != tc::OK) {
            std::printf("{\"code\": %d}\n", rc);
            return 0;
        }
        std::printf("{\"code\": 0, \"width\": %u, \"height\": %u, \"samples\": %u, \"bits\": %u, \"compression\": %u, \"photometric\": %u, "
                    "\"predictor\": %u, \"rows_per_strip\": %u, \"focal\": %u, \"little\": %s, \"row_bytes\": %llu, \"tile\": [%u, %u, %u, %u], ",
                    h.width, h.height, h.samples, h.bits, h.compression, h.photometric, h.predictor, h.rows_per_strip, h.focal_length_35mm,
                    h.little ? "true" : "false", (unsigned long long)h.row_bytes, h.tile_width, h.tile_length, h.tiles_across, h.tiles_down);
        std::printf("\"sem\": %s, \"scale\": [%" PRIu32 ", %" PRIu32 "], \"tilt\": %s%" PRIu32 ", \"databar\": %" PRIu32, h.sem ? "true" : "false",
                    f32_bits(h.scale[0]), f32_bits(h.scale[1]), h.have_tilt ? "" : "-", h.have_tilt ? f32_bits(h.tilt_angle) : 1u, h.databar_height);
        std::printf(", \"streams\": [");
        for (size_t s = 0; s < h.strips.size(); s++) {
            const tc::Strip &t = h.strips[s];
            std::printf("%s[%u, %u, %u, %u, %u, %u]", s ? ", " : "", t.offset, t.count, t.rows, t.row_bytes, t.x, t.y);
        }
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
            tc::Header h;
            const int rc = run(bytes, h);
            if (rc != tc::OK && rc != tc::INVALID && rc != tc::UNSUPPORTED) std::abort();
            counts[rc == tc::OK ? 0 : rc == tc::INVALID ? 1 : 2]++;
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
