// host_png_ext: the PNG decoder that reads Adam7 files too, through the C++ host layer (cvhip_host.hpp, namespace image:
// png_ext_info, png_ext_decode, calibration_matrix).
// usage: host_png_ext <file.png> <drop_rows> <luma.bin> <rgb.bin>   - prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const uint32_t drop_rows = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    try {
        using namespace cvhip_host;
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const image::PngInfo info = image::png_ext_info(file.data(), file.size());
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        const std::vector<uint8_t> luma = image::png_ext_decode(dev, file.data(), file.size(), image::Format::Luma8, drop_rows);
        const std::vector<uint8_t> rgb = image::png_ext_decode(dev, file.data(), file.size(), image::Format::Rgb8, drop_rows);
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char *>(luma.data()), (std::streamsize)luma.size());
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(rgb.data()), (std::streamsize)rgb.size());
        const std::array<double, 9> k = image::calibration_matrix(info.width, info.height - drop_rows, info.focal_length_35mm);
        // what the entry points that do not read interlaced files say of this one: the code, as an exception
        int old_code = 0;
        try {
            image::png_decode(dev, file.data(), file.size());
        } catch (const GpuError &e) {
            old_code = e.code;
        }
        std::printf("{\"info\": [%u, %u, %u, %u, %u, %u, %u, %u], \"old_code\": %d, \"k\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}\n",
                    info.width, info.height, info.colour_type, info.bit_depth, info.interlace, info.idat_chunks, info.focal_length_35mm,
                    (unsigned)info.plte | (unsigned)info.trns << 1, old_code, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8]);
        // a file that is cut short is refused with a message, as an exception
        try {
            image::png_ext_decode(dev, file.data(), file.size() / 2);
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
