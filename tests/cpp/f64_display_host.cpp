// f64_display_host.cpp — cybervision_amd/csrc/f64_display.hpp as plain C++ on the CPU (tests/test_f64_display_host_cpu.py
// builds it with AddressSanitizer and UBSan).
//   f64_display_host values.bin strings.txt lengths.bin
// values.bin: doubles.  strings.txt receives `{}` of each, one per line; lengths.bin what the length function says, as uint32.
// Every line is written into a buffer of exactly the length function's size (the sanitizer sees one byte more), the digits are
// cross-checked against std::to_chars(..., scientific), the integer pair against std::to_string.  Exit code 1 on a difference.
//   f64_display_host --time values.bin     prints the seconds one thread takes to write "v x y z\n" for each three doubles
#include <charconv>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../cybervision_amd/csrc/f64_display.hpp"

namespace fd = f64_display;

static std::vector<double> read_doubles(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) std::perror(path), std::exit(2);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<double> v((size_t)bytes / sizeof(double));
    if (!v.empty() && std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

// digits and exponent of std::to_chars' shortest scientific form: "d.ddde+XX" -> (ddd without trailing zeros, exponent of the last digit)
static bool to_chars_agrees(double v, const fd::Decimal &d)
{
    char buf[64];
    const auto res = std::to_chars(buf, buf + sizeof(buf), std::fabs(v), std::chars_format::scientific);
    const std::string s(buf, res.ptr);
    const size_t e = s.find('e');
    uint64_t digits = 0;
    int after_point = 0;
    bool seen_point = false;
    for (size_t i = 0; i < e; i++) {
        if (s[i] == '.') {
            seen_point = true;
            continue;
        }
        digits = digits * 10 + (uint64_t)(s[i] - '0');
        after_point += seen_point ? 1 : 0;
    }
    int exp10 = std::atoi(s.c_str() + e + 1) - after_point;
    while (digits && digits % 10 == 0) digits /= 10, exp10++;
    if (digits == 0) return d.digits == 0;
    return digits == d.digits && exp10 == d.exp10;
}

static int time_lines(const std::vector<double> &v)
{
    std::vector<char> out(3 * 330 + 8);
    uint64_t bytes = 0, mix = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i + 2 < v.size(); i += 3) {
        char *p = out.data();
        *p++ = 'v';
        for (int j = 0; j < 3; j++) *p++ = ' ', p += fd::f64_write(p, v[i + j]);
        *p++ = '\n';
        bytes += (uint64_t)(p - out.data()), mix += (uint8_t)p[-2];
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"lines\": %zu, \"bytes\": %" PRIu64 ", \"seconds\": %.6f, \"mix\": %" PRIu64 "}\n", v.size() / 3, bytes, seconds, mix);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--time") return time_lines(read_doubles(argv[2]));
    if (argc != 4) return std::fprintf(stderr, "usage: f64_display_host values.bin strings.txt lengths.bin\n"), 2;
    const std::vector<double> values = read_doubles(argv[1]);
    std::FILE *fs = std::fopen(argv[2], "wb"), *fl = std::fopen(argv[3], "wb");
    if (!fs || !fl) return 2;
    int bad = 0;
    std::vector<uint32_t> lengths(values.size());
    for (size_t i = 0; i < values.size(); i++) {
        const double v = values[i];
        const uint32_t len = fd::f64_len(v);
        std::unique_ptr<char[]> line(new char[len + 1]); // exactly the promised size, so that a byte past it is an ASan report
        const uint32_t wrote = fd::f64_write(line.get(), v);
        line[len] = '\n';
        lengths[i] = len;
        const fd::Decimal d = fd::shortest(v);
        if (wrote != len || (d.kind == fd::FINITE && !to_chars_agrees(v, d))) {
            if (bad++ < 10) std::fprintf(stderr, "value %zu (%a): length %u, wrote %u, or digits differ from std::to_chars\n", i, v, len, wrote);
        }
        std::fwrite(line.get(), 1, len + 1, fs);
    }
    std::fwrite(lengths.data(), sizeof(uint32_t), lengths.size(), fl);
    std::fclose(fs), std::fclose(fl);
    // the integer pair
    const uint64_t ints[] = {0, 1, 9, 10, 99, 100, 12941, 4294967295ull, 4294967296ull, 9999999999999999ull, 10000000000000000ull,
                             99999999999999999ull, 18446744073709551615ull};
    for (const uint64_t v : ints) {
        const std::string want = std::to_string(v);
        std::unique_ptr<char[]> text(new char[fd::u64_len(v)]);
        const uint32_t wrote = fd::u64_write(text.get(), v);
        if (fd::u64_len(v) != want.size() || wrote != want.size() || std::string(text.get(), wrote) != want) {
            std::fprintf(stderr, "integer %" PRIu64 " differs from std::to_string\n", v);
            bad++;
        }
    }
    std::printf("{\"values\": %zu, \"bad\": %d}\n", values.size(), bad);
    return bad ? 1 : 0;
}
