// tiff_out_host: cybervision_amd/csrc/tiff_encode_common.hpp as plain C++ on the CPU (built with sanitizers by
// tests/test_tiff_out_host_cpu.py, which compares with tests/ref_tiff_out.py).
//   tiff_out_host plan <w> <h> <channels> <compression> <predictor> <rows_per_strip> <first_count> <out.bin>
//                                  the refusal (u32: 0 accepted, 1 invalid, 2 unsupported); when accepted: row_bytes, rows per
//                                  strip, strips, offsets_at, counts_at, data_at (6 u32), worst_strip of a full strip and the size
//                                  of the file were it uncompressed (2 u64), then the header's bytes
//   tiff_out_host widths <out.bin> lzw_code_width(0 .. 4095) as bytes
//   tiff_out_host lzw <in.bin> <out.bin>       the LZW stream of the file's bytes as one strip, walked by lzw_byte / lzw_finish
//                                  against a table of LZW_SLOTS in a buffer of exactly worst_strip bytes; then codes and Clears (2 u32)
//   tiff_out_host packbits <row_bytes> <in.bin> <out.bin>   per row of the file: the size (u32), the packets (u32), the bytes -
//                                  each row from a buffer of exactly its size into one of exactly the bound
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/tiff_encode_common.hpp"

namespace te = tiff_encode_common;

static std::vector<uint8_t> load(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <typename T> static void put(std::vector<uint8_t> &out, T v)
{
    const uint8_t *b = reinterpret_cast<const uint8_t *>(&v);
    out.insert(out.end(), b, b + sizeof(T));
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
    auto number = [&](int k) { return (uint32_t)std::strtoul(argv[k], nullptr, 10); };
    std::vector<uint8_t> out;
    if (mode == "plan" && argc == 10) {
        te::Layout l;
        const te::Refusal r = te::plan(number(2), number(3), number(4), number(5), number(6), number(7), l);
        put<uint32_t>(out, (uint32_t)r);
        if (r == te::ACCEPTED) {
            for (uint32_t v : {l.row_bytes, l.rows_per_strip, l.strips, l.offsets_at, l.counts_at, l.data_at}) put<uint32_t>(out, v);
            put<uint64_t>(out, te::worst_strip(l.compression, l.rows_per_strip, l.row_bytes));
            put<uint64_t>(out, te::raw_file_size(l));
            const std::vector<uint8_t> h = te::header(l, number(8));
            out.insert(out.end(), h.begin(), h.end());
        }
        return save(argv[9], out);
    }
    if (mode == "widths" && argc == 3) {
        for (uint32_t c = 0; c < 4096; c++) out.push_back((uint8_t)te::lzw_code_width(c));
        return save(argv[2], out);
    }
    if (mode == "lzw" && argc == 4) {
        const std::vector<uint8_t> in = load(argv[2]);
        const size_t cap = (size_t)te::worst_strip(te::COMPRESSION_LZW, 1, in.size());
        std::unique_ptr<uint8_t[]> stream(new uint8_t[cap]()); // exactly the bound: a byte past it is the sanitizer's
        std::unique_ptr<uint32_t[]> table(new uint32_t[te::LZW_SLOTS]);
        auto empty = [&]() {
            for (uint32_t k = 0; k < te::LZW_SLOTS; k++) table[k] = te::LZW_EMPTY;
        };
        empty();
        uint64_t bits = 0;
        uint32_t codes = 0, clears = 0;
        auto emit = [&](uint32_t code, uint32_t width) {
            for (uint32_t b = 0; b < width; b++, bits++)
                if ((code >> (width - 1 - b)) & 1u) stream[bits >> 3] |= (uint8_t)(0x80u >> (bits & 7u));
            codes++;
            if (code == te::LZW_CLEAR) clears++;
        };
        te::LzwState st;
        emit(te::LZW_CLEAR, 9);
        for (uint8_t byte : in)
            if (te::lzw_byte(table.get(), st, byte, emit)) empty();
        te::lzw_finish(st, emit);
        out.assign(stream.get(), stream.get() + (bits + 7) / 8);
        put<uint32_t>(out, codes);
        put<uint32_t>(out, clears);
        return save(argv[3], out);
    }
    if (mode == "packbits" && argc == 5) {
        const uint32_t row_bytes = number(2);
        const std::vector<uint8_t> in = load(argv[3]);
        if (!row_bytes || in.size() % row_bytes) return 2;
        const size_t cap = (size_t)te::worst_strip(te::COMPRESSION_PACKBITS, 1, row_bytes);
        for (size_t at = 0; at < in.size(); at += row_bytes) {
            std::unique_ptr<uint8_t[]> row(new uint8_t[row_bytes]), packed(new uint8_t[cap]);
            std::memcpy(row.get(), in.data() + at, row_bytes);
            uint32_t packets = 0;
            const uint32_t size = te::packbits_row(row.get(), row_bytes, packed.get(), packets);
            if (size > cap) return 3;
            put<uint32_t>(out, size);
            put<uint32_t>(out, packets);
            out.insert(out.end(), packed.get(), packed.get() + size);
        }
        return save(argv[4], out);
    }
    return 2;
}
