// cybervision_amd/csrc/jpeg_common.hpp on the CPU, built with AddressSanitizer and UBSan by tests/test_jpeg_host_cpu.py:
//   jpeg_host parse FILE            one line of JSON: the return code and, when it is 0, what the parser found, else the reason
//   jpeg_host fuzz FILE SEED FLIPS  the parser over every truncation of the file and over FLIPS seeded corruptions of
//                                   it; prints a CRC over every case's code and reason in order, then on the last line
//                                   how often each code came back
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/jpeg_common.hpp"

namespace jc = jpeg_common;

static std::vector<uint8_t> read_file(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

static uint32_t crc32(const uint8_t *data, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= data[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}

// the parser, and when it accepts the file every lookup the decoder would build -> the code
static int run(const std::vector<uint8_t> &data, jc::Header &h, std::vector<uint16_t> &lut)
{
    // (an exact-size copy: a read past the file's end is a read past the allocation)
    std::vector<uint8_t> exact(data.begin(), data.end());
    const int rc = jc::parse(exact.data(), exact.size(), h);
    if (rc != jc::OK) return rc;
    if (h.scan_begin > h.scan_end || h.scan_end > exact.size()) std::abort();
    for (uint32_t c = 0; c < h.components; c++) {
        jc::build_lut(h.huff[0][h.comp[c].td], lut.data());
        jc::build_lut(h.huff[1][h.comp[c].ta], lut.data());
    }
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> data = read_file(argv[2]);
    std::vector<uint16_t> lut(jc::LUT_ENTRIES);
    if (mode == "parse") {
        jc::Header h;
        const int rc = run(data, h, lut);
        if (rc != jc::OK) {
            std::printf("{\"code\": %d, \"reason\": \"%s\"}\n", rc, h.error);
            return 0;
        }
        std::printf("{\"code\": 0, \"width\": %u, \"height\": %u, \"components\": %u, \"hmax\": %u, \"vmax\": %u, \"mcus_x\": %u, \"mcus_y\": %u, "
                    "\"restart\": %u, \"focal\": %u, \"scan\": [%llu, %llu], \"segments\": %llu, \"bpm\": %u, \"comps\": [",
                    h.width, h.height, h.components, h.hmax, h.vmax, h.mcus_x, h.mcus_y, h.restart, h.focal_length_35mm,
                    (unsigned long long)h.scan_begin, (unsigned long long)h.scan_end, (unsigned long long)jc::segments(h), jc::blocks_per_mcu(h));
        for (uint32_t c = 0; c < h.components; c++) {
            const jc::Component &k = h.comp[c];
            std::printf("%s{\"id\": %u, \"h\": %u, \"v\": %u, \"tq\": %u, \"td\": %u, \"ta\": %u, \"quant\": [", c ? ", " : "", k.id, k.h, k.v, k.tq, k.td, k.ta);
            for (int i = 0; i < 64; i++) std::printf("%s%u", i ? ", " : "", h.quant[k.tq][i]);
            jc::build_lut(h.huff[0][k.td], lut.data());
            const uint32_t dc = crc32(reinterpret_cast<const uint8_t *>(lut.data()), lut.size() * 2);
            jc::build_lut(h.huff[1][k.ta], lut.data());
            std::printf("], \"dc_lut\": %u, \"ac_lut\": %u}", dc, crc32(reinterpret_cast<const uint8_t *>(lut.data()), lut.size() * 2));
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
        std::string reasons; // "code:reason\n" of every case
        auto tally = [&](const std::vector<uint8_t> &bytes) {
            jc::Header h;
            const int rc = run(bytes, h, lut);
            if (rc != jc::OK && rc != jc::INVALID && rc != jc::UNSUPPORTED) std::abort();
            reasons += std::to_string(rc) + ":" + h.error + "\n";
            counts[rc == jc::OK ? 0 : rc == jc::INVALID ? 1 : 2]++;
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
        std::printf("reasons %u\n%d %d %d\n", crc32(reinterpret_cast<const uint8_t *>(reasons.data()), reasons.size()), counts[0], counts[1], counts[2]);
        return 0;
    }
    return 2;
}
