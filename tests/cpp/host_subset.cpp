// host_subset: cvhip_surface_subset through the C++ host layer (cvhip_host.hpp, mesh::surface_subset).
// usage: host_subset <dir> <cameras> <max_points> <seed>   - reads <dir>/points.bin (n x 3 f64) and <dir>/tracks.bin
// (n x cameras x 2 i32), writes <dir>/out_points.bin, <dir>/out_tracks.bin and <dir>/out_rows.bin (u64) and prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

template <typename T> static std::vector<T> read_all(const std::string &path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T> static void write_all(const std::string &path, const std::vector<T> &v)
{
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const std::string dir = argv[1];
    try {
        using namespace cvhip_host;
        const uint32_t cameras = (uint32_t)std::strtoul(argv[2], nullptr, 10);
        const uint64_t max_points = std::strtoull(argv[3], nullptr, 10), seed = std::strtoull(argv[4], nullptr, 10);
        mesh::Surface s;
        s.points = read_all<double>(dir + "/points.bin");
        s.tracks = read_all<int32_t>(dir + "/tracks.bin");
        s.projection.assign(12 * (size_t)cameras, 0.0);
        s.r.assign(3 * (size_t)cameras, 0.0);
        s.t.assign(3 * (size_t)cameras, 0.0);
        s.image_dims.assign(2 * (size_t)cameras, 64);
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        std::vector<uint64_t> rows;
        const mesh::Surface out = mesh::surface_subset(dev, s, max_points, seed, &rows);
        write_all(dir + "/out_points.bin", out.points);
        write_all(dir + "/out_tracks.bin", out.tracks);
        write_all(dir + "/out_rows.bin", rows);
        std::printf("{\"rows_in\": %llu, \"rows_out\": %llu, \"cameras\": %u}\n", (unsigned long long)s.tracks_len(),
                    (unsigned long long)out.tracks_len(), out.cameras_len());
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
