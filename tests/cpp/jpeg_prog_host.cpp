// cybervision_amd/csrc/jpeg_prog_common.hpp on the CPU, built with AddressSanitizer and UBSan by tests/test_jpeg_prog_host_cpu.py:
//   jpeg_prog_host parse FILE            one line of JSON: the return code and, when the walk accepts the file, the frame, the
//                                        scan list with its lookups and intervals, and the entropy decode of every interval in
//                                        launch order (decode_interval, the device lane's text): its code and the block store;
//                                        else the walk's reason
//   jpeg_prog_host fuzz FILE SEED FLIPS  the same over every truncation of the file and over FLIPS seeded corruptions of it;
//                                        prints a CRC over every case's code and reason in order, then on the last line how
//                                        often each code came back
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/jpeg_prog_common.hpp"

namespace jp = jpeg_prog;
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

struct Result {
    jp::File f;
    std::vector<uint16_t> luts;
    std::vector<int16_t> coef;
    uint32_t met[jp::METS] = {0, 0, 0, 0};
    int decode = 0;
};

// the walk, and when it accepts the file every lookup and the entropy decode of every interval -> the code
static int run(const std::vector<uint8_t> &data, Result &r, size_t most_blocks)
{
    // (an exact-size copy: a read past the file's end is a read past the allocation)
    std::vector<uint8_t> exact(data.begin(), data.end());
    const int rc = jp::parse(exact.data(), exact.size(), r.f, true);
    if (rc != jp::OK) return rc;
    const jp::Frame &F = r.f.frame;
    const size_t blocks = (size_t)F.mcus_x * F.mcus_y * F.bpm;
    if (blocks > most_blocks) return rc; // (fuzz: a corrupted frame size - the store is the device's business)
    r.luts.assign(r.f.tables.size() * jc::LUT_ENTRIES, 0);
    for (size_t t = 0; t < r.f.tables.size(); t++) jc::build_lut(r.f.tables[t], r.luts.data() + t * jc::LUT_ENTRIES);
    r.coef.assign(blocks * 64, 0);
    uint32_t err = 0;
    for (const jp::Interval &iv : r.f.intervals) {
        if (iv.begin > iv.end || iv.end > exact.size() || iv.scan >= r.f.scans.size()) std::abort();
        err |= jp::decode_interval(exact.data(), F, r.f.scans[iv.scan], iv.index, iv.begin, iv.end, r.luts.data(), jc::ZIGZAG, r.coef.data(), r.met);
    }
    r.decode = err ? jp::INVALID : jp::OK;
    // the same decode from data bytes alone, as the device reads them from its clean buffer: the same store, the same code
    std::vector<uint8_t> clean;
    std::vector<int16_t> again(blocks * 64, 0);
    uint32_t err_again = 0, met_again[jp::METS] = {0, 0, 0, 0};
    std::vector<uint32_t> at(1, 0u);
    for (const jp::Interval &iv : r.f.intervals) {
        for (uint32_t i = iv.begin; i < iv.end;) {
            if (exact[i] != 0xFF) {
                clean.push_back(exact[i++]);
                continue;
            }
            uint32_t q = i + 1;
            while (q < iv.end && exact[q] == 0xFF) q++;
            if (q >= iv.end) break;
            clean.push_back(0xFF), i = q + 1; // (inside an interval a run of FF is followed by 00)
        }
        at.push_back((uint32_t)clean.size());
    }
    std::vector<uint8_t> tight(clean.begin(), clean.end());
    for (size_t k = 0; k < r.f.intervals.size(); k++) {
        const jp::Interval &iv = r.f.intervals[k];
        err_again |= jp::decode_interval(tight.data(), F, r.f.scans[iv.scan], iv.index, at[k], at[k + 1], r.luts.data(), jc::ZIGZAG, again.data(), met_again, false);
    }
    if ((err != 0) != (err_again != 0) || (!err && again != r.coef)) std::abort();
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> data = read_file(argv[2]);
    if (mode == "parse") {
        Result r;
        const int rc = run(data, r, (size_t)1 << 25);
        if (rc != jp::OK) {
            std::printf("{\"code\": %d, \"reason\": \"%s\"}\n", rc, r.f.error);
            return 0;
        }
        const jp::Frame &F = r.f.frame;
        std::printf("{\"code\": 0, \"width\": %u, \"height\": %u, \"components\": %u, \"hmax\": %u, \"vmax\": %u, \"mcus_x\": %u, \"mcus_y\": %u, \"bpm\": %u, "
                    "\"focal\": %u, \"subsequences\": %llu, \"ac_refinement_scans\": %u, \"quant\": [",
                    F.width, F.height, F.ncomp, F.hmax, F.vmax, F.mcus_x, F.mcus_y, F.bpm, r.f.focal_length_35mm, (unsigned long long)r.f.subsequences,
                    r.f.ac_refinement_scans);
        for (uint32_t c = 0; c < F.ncomp; c++) {
            std::printf("%s[", c ? ", " : "");
            for (int i = 0; i < 64; i++) std::printf("%s%u", i ? ", " : "", r.f.quant[c][i]);
            std::printf("]");
        }
        std::printf("], \"scans\": [");
        auto lut_crc = [&](uint32_t t) { return crc32(reinterpret_cast<const uint8_t *>(r.luts.data() + (size_t)t * jc::LUT_ENTRIES), jc::LUT_ENTRIES * 2); };
        for (size_t s = 0; s < r.f.scans.size(); s++) {
            const jp::Scan &S = r.f.scans[s];
            std::printf("%s{\"comps\": [", s ? ", " : "");
            for (uint32_t k = 0; k < S.ncomp; k++) std::printf("%s%u", k ? ", " : "", S.comp[k]);
            std::printf("], \"ss\": %u, \"se\": %u, \"ah\": %u, \"al\": %u, \"restart\": %u, \"mcus\": %u, \"level\": %u, \"dc_luts\": [", S.ss, S.se, S.ah, S.al,
                        S.restart, S.mcus, S.level);
            bool any = false;
            for (uint32_t k = 0; k < S.ncomp; k++)
                if (S.dc_lut[k] != jp::NO_LUT) std::printf("%s%u", any ? ", " : "", lut_crc(S.dc_lut[k])), any = true;
            std::printf("], \"ac_lut\": ");
            if (S.ac_lut != jp::NO_LUT) std::printf("%u", lut_crc(S.ac_lut));
            else std::printf("null");
            std::printf(", \"intervals\": [");
            for (uint32_t k = 0; k < S.intervals; k++) {
                const jp::Interval &iv = r.f.intervals[S.first_interval + k];
                if (iv.scan != s || iv.index != k) std::abort();
                std::printf("%s[%u, %u]", k ? ", " : "", iv.begin, iv.end);
            }
            std::printf("]}");
        }
        std::printf("], \"decode\": %d, \"coef\": %u, \"met\": [%u, %u, %u, %u]}\n", r.decode,
                    crc32(reinterpret_cast<const uint8_t *>(r.coef.data()), r.coef.size() * 2), r.met[0], r.met[1], r.met[2], r.met[3]);
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
        std::string reasons; // "code:reason\n" of every case (the walk's reason: none where only the entropy decode refuses)
        auto tally = [&](const std::vector<uint8_t> &bytes) {
            Result r;
            int rc = run(bytes, r, (size_t)1 << 16);
            if (rc == jp::OK) rc = r.decode;
            if (rc != jp::OK && rc != jp::INVALID && rc != jp::UNSUPPORTED) std::abort();
            reasons += std::to_string(rc) + ":" + r.f.error + "\n";
            counts[rc == jp::OK ? 0 : rc == jp::INVALID ? 1 : 2]++;
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
