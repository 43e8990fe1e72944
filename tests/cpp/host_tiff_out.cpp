// host_tiff_out: the TIFF encoder through the C++ host layer (cvhip_host.hpp, namespace mesh: tiff_encode).
// usage: host_tiff_out <pixels.bin> <width> <height> <channels> <compression> <predictor> <rows_per_strip> <out.tif>   - prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) return 2;
    auto number = [&](int k) { return (uint32_t)std::strtoul(argv[k], nullptr, 10); };
    const uint32_t width = number(2), height = number(3), channels = number(4), compression = number(5), predictor = number(6), rps = number(7);
    try {
        using namespace cvhip_host;
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> pixels((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (pixels.size() != (size_t)width * height * channels) throw std::runtime_error("bad input size");
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        mesh::TiffSections sec;
        const std::vector<uint8_t> file = mesh::tiff_encode(dev, pixels.data(), width, height, channels, (mesh::TiffCompression)compression, predictor, rps, &sec);
        const mesh::TiffEncodeStats st = mesh::tiff_encode_last_stats();
        std::ofstream out(argv[8], std::ios::binary);
        out.write(reinterpret_cast<const char *>(file.data()), (std::streamsize)file.size());
        std::printf("{\"size\": %zu, \"sections\": [%llu, %llu, %llu], \"stats\": [%llu, %llu, %llu, %llu]}\n", file.size(),
                    (unsigned long long)sec.before, (unsigned long long)sec.strips, (unsigned long long)sec.after, (unsigned long long)st.strips,
                    (unsigned long long)st.codes, (unsigned long long)st.clears, (unsigned long long)st.packets);
        // arguments the library does not take are refused with a message, as an exception
        try {
            mesh::tiff_encode(dev, pixels.data(), width, height, channels, mesh::TiffCompression::PackBits, 2);
            return 3;
        } catch (const GpuError &e) {
            if (e.code != CVHIP_ERR_INVALID) return 4;
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
