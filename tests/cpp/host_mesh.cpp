// host_mesh: the mesh stage through the C++ host layer (cvhip_host.hpp, namespace mesh).
// usage: host_mesh <dir> <n> <m>   - reads <dir>/points.bin (n x 3 f64), tracks.bin (n x m x 2 i32), cameras.bin (m x (12 + 3 +
// 3) f64: projection, r, t), dims.bin (m x 2 u32) and faces<i>.bin (u32 triples into camera i's points: the caller's
// Delaunay); writes polygons.bin (u32 x 3), camera.bin (u32), map.bin (f64) and prints one JSON line.
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
    const size_t bytes = (size_t)f.tellg();
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T> static void write_all(const std::string &path, const T *data, size_t count)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(data), (std::streamsize)(count * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::string dir = argv[1];
    const size_t n = std::strtoull(argv[2], nullptr, 10), m = std::strtoull(argv[3], nullptr, 10);
    try {
        using namespace cvhip_host;
        mesh::Surface s;
        s.points = read_all<double>(dir + "/points.bin");
        s.tracks = read_all<int32_t>(dir + "/tracks.bin");
        s.image_dims = read_all<uint32_t>(dir + "/dims.bin");
        const std::vector<double> cams = read_all<double>(dir + "/cameras.bin");
        if (s.points.size() != 3 * n || s.tracks.size() != 2 * n * m || cams.size() != 18 * m) throw std::runtime_error("bad input sizes");
        for (size_t j = 0; j < m; j++) {
            s.projection.insert(s.projection.end(), cams.begin() + 18 * j, cams.begin() + 18 * j + 12);
            s.r.insert(s.r.end(), cams.begin() + 18 * j + 12, cams.begin() + 18 * j + 15);
            s.t.insert(s.t.end(), cams.begin() + 18 * j + 15, cams.begin() + 18 * j + 18);
        }
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        uint32_t camera = 0;
        size_t points0 = 0;
        mesh::Mesh result = mesh::Mesh::create(dev, s, [&](const mesh::CameraPoints &cp) {
            if (camera == 0) points0 = cp.track_i.size();
            return read_all<uint32_t>(dir + "/faces" + std::to_string(camera++) + ".bin");
        });
        std::vector<uint32_t> polys, cam;
        for (const mesh::Polygon &p : result.polygons) {
            polys.insert(polys.end(), p.vertices.begin(), p.vertices.end());
            cam.push_back(p.camera_i);
        }
        write_all(dir + "/polygons.bin", polys.data(), polys.size());
        write_all(dir + "/camera.bin", cam.data(), cam.size());
        const mesh::DepthImage img = mesh::depth_image(dev, s, 0, -1.0, result.polygons);
        write_all(dir + "/map.bin", img.map.data(), img.map.width() * img.map.height());
        std::printf("{\"polygons\": %zu, \"points0\": %zu, \"width\": %zu, \"height\": %zu, \"min_x\": %.17g, \"min_y\": %.17g, "
                    "\"min_depth\": %.17g, \"max_depth\": %.17g}\n",
                    result.polygons.size(), points0, img.map.width(), img.map.height(), img.min_x, img.min_y, img.min_depth, img.max_depth);
        // an affine surface (no cameras) is refused with a message, as an exception
        mesh::Surface none;
        none.points = s.points;
        try {
            mesh::cull(dev, none, 0, polys);
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
