// host_tiff_ext: Deflate and tiled TIFF files through the C++ host layer (cvhip_host.hpp, namespace image: tiff_ext_info, tiff_ext_decode).
// usage: host_tiff_ext <file.tif> <drop_rows or -1 for the file's databar> <luma.bin> <rgb.bin>   - prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const long drop = std::strtol(argv[2], nullptr, 10);
    try {
        using namespace cvhip_host;
        const uint32_t drop_rows = drop < 0 ? image::DROP_DATABAR : (uint32_t)drop;
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const image::TiffExtInfo info = image::tiff_ext_info(file.data(), file.size());
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        const std::vector<uint8_t> luma = drop < 0 ? image::tiff_ext_decode(dev, file.data(), file.size())
                                                   : image::tiff_ext_decode(dev, file.data(), file.size(), image::Format::Luma8, drop_rows);
        const std::vector<uint8_t> rgb = image::tiff_ext_decode(dev, file.data(), file.size(), image::Format::Rgb8, drop_rows);
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char *>(luma.data()), (std::streamsize)luma.size());
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(rgb.data()), (std::streamsize)rgb.size());
        uint32_t scale[2];
        std::memcpy(scale, info.scale, 8);
        std::printf("{\"width\": %u, \"height\": %u, \"samples\": %u, \"bits\": %u, \"compression\": %u, \"photometric\": %u, \"predictor\": %u, "
                    "\"strips\": %u, \"rows_per_strip\": %u, \"focal\": %u, \"databar\": %u, \"sem\": %s, \"has_tilt\": %s, \"scale\": [%u, %u], "
                    "\"tile_width\": %u, \"tile_length\": %u, \"tiles_across\": %u}\n",
                    info.width, info.height, info.samples, info.bits, info.compression, info.photometric, info.predictor, info.strips,
                    info.rows_per_strip, info.focal_length_35mm, info.databar_height, info.sem ? "true" : "false",
                    info.has_tilt_angle ? "true" : "false", scale[0], scale[1], info.tile_width, info.tile_length, info.tiles_across);
        // the old entry point still refuses the file, as an exception
        try {
            image::tiff_decode(dev, file.data(), file.size());
            return 3;
        } catch (const GpuError &e) {
            if (e.code != CVHIP_ERR_UNSUPPORTED) return 4;
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
