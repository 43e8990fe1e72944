// png_host.cpp — cybervision_amd/csrc/png_common.hpp as plain C++ on the CPU, for tests/test_png_host_cpu.py (built with
// AddressSanitizer and UBSan).
//   png_host codes IN OUT     IN: histograms of 286 uint64 each.  OUT, per histogram: 286 code lengths, 19 code-length-code
//                             lengths, then as uint32: hlit, hclen, the header's bits, its bytes; the header's bytes; the 513
//                             token table words.
//   png_host sums BUF SPLITS  BUF: bytes.  SPLITS: text, one case per line: ascending cut positions.  Prints per case
//                             "crc adler" of the whole buffer, combined from the values of its pieces.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../cybervision_amd/csrc/png_common.hpp"

namespace pc = png_common;

static std::vector<uint8_t> read_all(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static void put32(std::vector<uint8_t> &out, uint32_t v)
{
    for (int k = 0; k < 4; k++) out.push_back((uint8_t)(v >> (8 * k)));
}

static int run_codes(const char *in_path, const char *out_path)
{
    const std::vector<uint8_t> raw = read_all(in_path);
    const size_t each = pc::LITLEN_SYMBOLS * sizeof(uint64_t);
    if (raw.size() % each) return 2;
    std::vector<uint8_t> out;
    for (size_t at = 0; at < raw.size(); at += each) {
        uint64_t hist[pc::LITLEN_SYMBOLS];
        for (uint32_t s = 0; s < pc::LITLEN_SYMBOLS; s++) {
            hist[s] = 0;
            for (int k = 0; k < 8; k++) hist[s] |= (uint64_t)raw[at + 8 * s + k] << (8 * k);
        }
        const pc::BlockCodes bc = pc::block_codes(hist);
        out.insert(out.end(), bc.lengths.begin(), bc.lengths.end());
        out.insert(out.end(), bc.cl_lengths.begin(), bc.cl_lengths.end());
        put32(out, bc.hlit);
        put32(out, bc.hclen);
        put32(out, (uint32_t)bc.header.nbits);
        put32(out, (uint32_t)bc.header.bytes.size());
        out.insert(out.end(), bc.header.bytes.begin(), bc.header.bytes.end());
        for (uint32_t t = 0; t < pc::TOKENS; t++) put32(out, bc.table[t]);
    }
    std::ofstream f(out_path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    return f ? 0 : 2;
}

static int run_sums(const char *buf_path, const char *splits_path)
{
    const std::vector<uint8_t> buf = read_all(buf_path);
    std::ifstream splits(splits_path);
    std::string line;
    while (std::getline(splits, line)) {
        std::istringstream words(line);
        std::vector<size_t> cuts{0};
        size_t c;
        while (words >> c) cuts.push_back(c);
        cuts.push_back(buf.size());
        uint32_t crc = 0; // of nothing
        pc::AdlerSums sums{0, 0};
        for (size_t k = 0; k + 1 < cuts.size(); k++) {
            if (cuts[k + 1] < cuts[k] || cuts[k + 1] > buf.size()) return 2;
            const uint8_t *piece = buf.data() + cuts[k];
            const size_t n = cuts[k + 1] - cuts[k];
            crc = pc::crc_combine(crc, pc::crc32(piece, n), n);
            pc::AdlerSums own{0, 0};
            for (size_t i = 0; i < n; i++) {
                own.a = (own.a + piece[i]) % pc::ADLER_MOD;
                own.b = (uint32_t)((own.b + (uint64_t)((n - i) % pc::ADLER_MOD) * piece[i]) % pc::ADLER_MOD);
            }
            sums = pc::adler_join(sums, own, n);
        }
        std::printf("%u %u\n", crc, pc::adler_value(sums, buf.size()));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "codes") return run_codes(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "sums") return run_sums(argv[2], argv[3]);
    std::fprintf(stderr, "usage: png_host codes IN OUT | png_host sums BUF SPLITS\n");
    return 2;
}
