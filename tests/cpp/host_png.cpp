// host_png: the PNG encoder through the C++ host layer (cvhip_host.hpp, namespace mesh: png_encode).
// usage: host_png <pixels.bin> <width> <height> <channels> <filter> <out.png>   - prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    const uint32_t width = (uint32_t)std::strtoul(argv[2], nullptr, 10), height = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    const uint32_t channels = (uint32_t)std::strtoul(argv[4], nullptr, 10), filter = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    try {
        using namespace cvhip_host;
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> pixels((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (pixels.size() != (size_t)width * height * channels) throw std::runtime_error("bad input size");
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        mesh::PngSections sec;
        const std::vector<uint8_t> file = mesh::png_encode(dev, pixels.data(), width, height, channels, (mesh::PngFilter)filter, &sec);
        std::ofstream out(argv[6], std::ios::binary);
        out.write(reinterpret_cast<const char *>(file.data()), (std::streamsize)file.size());
        std::printf("{\"size\": %zu, \"sections\": [%llu, %llu, %llu]}\n", file.size(), (unsigned long long)sec.before,
                    (unsigned long long)sec.idat, (unsigned long long)sec.after);
        // arguments the library does not take are refused with a message, as an exception
        try {
            mesh::png_encode(dev, pixels.data(), width, height, 5, mesh::PngFilter::Adaptive);
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
