// host_delaunay: cvhip_mesh_delaunay through the C++ host layer (cvhip_host.hpp, mesh::delaunay).
// usage: host_delaunay <dir>   - reads <dir>/xy.bin (k x 2 f64), writes <dir>/faces.bin (u32 triples) and prints one JSON line.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    try {
        using namespace cvhip_host;
        std::ifstream f(dir + "/xy.bin", std::ios::binary | std::ios::ate);
        if (!f) throw std::runtime_error("cannot open xy.bin");
        std::vector<double> xy((size_t)f.tellg() / sizeof(double));
        f.seekg(0);
        f.read(reinterpret_cast<char *>(xy.data()), (std::streamsize)(xy.size() * sizeof(double)));
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        mesh::DelaunayStats st;
        const std::vector<uint32_t> faces = mesh::delaunay(dev, xy, &st);
        std::ofstream out(dir + "/faces.bin", std::ios::binary);
        out.write(reinterpret_cast<const char *>(faces.data()), (std::streamsize)(faces.size() * sizeof(uint32_t)));
        std::printf("{\"points\": %zu, \"faces\": %zu, \"device_stars\": %llu, \"host_stars\": %llu}\n", xy.size() / 2, faces.size() / 3,
                    (unsigned long long)st.device_stars, (unsigned long long)st.host_stars);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
