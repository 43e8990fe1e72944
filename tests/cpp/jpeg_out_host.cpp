// jpeg_out_host: cybervision_amd/csrc/jpeg_encode_common.hpp as plain C++ on the CPU (built with sanitizers by
// tests/test_jpeg_out_host_cpu.py, which compares with tests/ref_jpeg_out.py).
//   jpeg_out_host quant <out.bin>                 the luma and the chroma table, 64 bytes each, for quality 1 .. 100
//   jpeg_out_host tables <hist.bin> <out.bin>     hist.bin: records of 256 u64 counts; per record: the unfolded longest length
//                                                 (u32), bits[16], the number of values (u32), values[256], the code table
//                                                 code_table gives for 256 symbols (256 u32)
//   jpeg_out_host kernel_table <out.bin>          kernel_table of the four Annex K tables (TABLE_ENTRIES u32)
//   jpeg_out_host header <w> <h> <channels> <quality> <sampling> <hist.bin or -> <out.bin>
//                                                 SOI .. SOS with the Annex K tables (-) or the optimal tables of the file's
//                                                 2 or 4 records; then geometry: 11 u32 and the blocks and dummy blocks (2 u64)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/jpeg_encode_common.hpp"

namespace je = jpeg_encode_common;

static std::vector<uint64_t> read_u64(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<uint64_t> v(raw.size() / 8);
    std::memcpy(v.data(), raw.data(), v.size() * 8);
    return v;
}
template <typename T> static void put(std::vector<uint8_t> &out, const T *p, size_t n)
{
    const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
    out.insert(out.end(), b, b + n * sizeof(T));
}
static int save(const char *path, const std::vector<uint8_t> &out)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    return f.good() ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    std::vector<uint8_t> out;
    if (mode == "quant" && argc == 3) {
        for (uint32_t q = 1; q <= 100; q++) {
            uint16_t t[64];
            for (const uint8_t *base : {je::QUANT_LUMA, je::QUANT_CHROMA}) {
                je::quant_table(base, q, t);
                for (int i = 0; i < 64; i++) out.push_back((uint8_t)t[i]), out.push_back((uint8_t)(t[i] >> 8));
            }
        }
        return save(argv[2], out);
    }
    if (mode == "tables" && argc == 4) {
        const std::vector<uint64_t> hist = read_u64(argv[2]);
        if (hist.size() % 256) return 2;
        for (size_t r = 0; r < hist.size() / 256; r++) {
            uint32_t longest = 0, entries[256];
            const je::HuffSpec s = je::optimal_table(hist.data() + 256 * r, &longest);
            je::code_table(s, entries, 256);
            put(out, &longest, 1);
            put(out, s.bits, 16);
            put(out, &s.total, 1);
            put(out, s.values, 256);
            put(out, entries, 256);
        }
        return save(argv[3], out);
    }
    if (mode == "kernel_table" && argc == 3) {
        je::HuffSpec specs[4];
        for (uint32_t k = 0; k < 4; k++) specs[k] = je::standard_table(k);
        uint32_t table[je::TABLE_ENTRIES];
        je::kernel_table(specs, 4, table);
        put(out, table, je::TABLE_ENTRIES);
        return save(argv[2], out);
    }
    if (mode == "header" && argc == 9) {
        auto number = [&](int k) { return (uint32_t)std::strtoul(argv[k], nullptr, 10); };
        const je::Geometry g = je::geometry(number(2), number(3), number(4), number(6));
        uint16_t quants[2][64];
        je::quant_table(je::QUANT_LUMA, number(5), quants[0]);
        je::quant_table(je::QUANT_CHROMA, number(5), quants[1]);
        const uint32_t n_specs = g.components == 3 ? 4 : 2;
        je::HuffSpec specs[4];
        for (uint32_t k = 0; k < n_specs; k++) specs[k] = je::standard_table(k);
        if (std::string(argv[7]) != "-") {
            const std::vector<uint64_t> hist = read_u64(argv[7]);
            if (hist.size() != 256 * (size_t)n_specs) return 2;
            for (uint32_t k = 0; k < n_specs; k++) specs[k] = je::optimal_table(hist.data() + 256 * k);
        }
        out = je::header(g, quants, specs);
        const uint32_t geo[11] = {g.width, g.height, g.channels, g.components, g.hs, g.vs, g.mcus_x, g.mcus_y, g.blocks_x, g.blocks_y, g.bpm};
        const uint64_t counts[2] = {je::total_blocks(g), je::dummy_blocks(g)};
        put(out, geo, 11);
        put(out, counts, 2);
        return save(argv[8], out);
    }
    return 2;
}
