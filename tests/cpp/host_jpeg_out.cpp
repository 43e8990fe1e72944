// host_jpeg_out: the JPEG encoder through the C++ host layer (cvhip_host.hpp, namespace mesh: jpeg_encode).
// usage: host_jpeg_out <pixels.bin> <width> <height> <channels> <quality> <sampling> <optimize> <out.jpg>   - prints one JSON line.
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
    const uint32_t width = number(2), height = number(3), channels = number(4), quality = number(5), sampling = number(6), optimize = number(7);
    try {
        using namespace cvhip_host;
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> pixels((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (pixels.size() != (size_t)width * height * channels) throw std::runtime_error("bad input size");
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        mesh::JpegSections sec;
        const std::vector<uint8_t> file =
            mesh::jpeg_encode(dev, pixels.data(), width, height, channels, quality, (mesh::JpegSampling)sampling, optimize != 0, &sec);
        const mesh::JpegEncodeStats st = mesh::jpeg_encode_last_stats();
        std::ofstream out(argv[8], std::ios::binary);
        out.write(reinterpret_cast<const char *>(file.data()), (std::streamsize)file.size());
        std::printf("{\"size\": %zu, \"sections\": [%llu, %llu, %llu], \"stats\": [%llu, %llu, %llu, %llu]}\n", file.size(),
                    (unsigned long long)sec.before, (unsigned long long)sec.data, (unsigned long long)sec.after, (unsigned long long)st.blocks,
                    (unsigned long long)st.dummy_blocks, (unsigned long long)st.bits, (unsigned long long)st.stuffed);
        // arguments the library does not take are refused with a message, as an exception
        try {
            mesh::jpeg_encode(dev, pixels.data(), width, height, channels, 101);
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
