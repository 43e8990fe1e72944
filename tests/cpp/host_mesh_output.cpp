// host_mesh_output: the mesh output through the C++ host layer (cvhip_host.hpp, namespace mesh: ply, colour_map).
// usage: host_mesh_output <dir> <n> <m>   - reads <dir>/points.bin (n x 3 f64), tracks.bin (n x m x 2 i32), polygons.bin (u32
// triples), images.bin (the m RGB8 images, concatenated), dims.bin (m x 2 u32: width, height), scale.bin (3 f64), map.bin (f64,
// mapdims.bin: width, height u32; minmax.bin 2 f64) and table.bin (768 u8); writes plain.ply, color.ply, rgba.bin and prints
// one JSON line.
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
        mesh::Surface s; // (no cameras: the writer does not touch them)
        s.points = read_all<double>(dir + "/points.bin");
        s.tracks = read_all<int32_t>(dir + "/tracks.bin");
        if (s.points.size() != 3 * n || s.tracks.size() != 2 * n * m) throw std::runtime_error("bad input sizes");
        const std::vector<uint32_t> flat = read_all<uint32_t>(dir + "/polygons.bin"), dims = read_all<uint32_t>(dir + "/dims.bin");
        const std::vector<uint8_t> pixels = read_all<uint8_t>(dir + "/images.bin");
        const std::vector<double> scale = read_all<double>(dir + "/scale.bin");
        std::vector<mesh::Polygon> polygons;
        for (size_t p = 0; p + 2 < flat.size(); p += 3) polygons.push_back(mesh::Polygon{0, {flat[p], flat[p + 1], flat[p + 2]}});
        std::vector<mesh::RgbImage> images(m);
        size_t at = 0;
        for (size_t c = 0; c < m; c++) {
            images[c].width = dims[2 * c], images[c].height = dims[2 * c + 1];
            const size_t bytes = (size_t)images[c].width * images[c].height * 3;
            images[c].pixels.assign(pixels.begin() + at, pixels.begin() + at + bytes);
            at += bytes;
        }
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        const std::array<double, 3> out_scale{scale.at(0), scale.at(1), scale.at(2)};
        mesh::PlySections plain_sec, color_sec;
        const std::vector<uint8_t> plain = mesh::ply(dev, s, polygons, {}, mesh::VertexMode::Plain, out_scale, &plain_sec);
        const std::vector<uint8_t> color = mesh::ply(dev, s, polygons, images, mesh::VertexMode::Color, out_scale, &color_sec);
        write_all(dir + "/plain.ply", plain.data(), plain.size());
        write_all(dir + "/color.ply", color.data(), color.size());
        const std::vector<uint32_t> map_dims = read_all<uint32_t>(dir + "/mapdims.bin");
        const std::vector<double> cells = read_all<double>(dir + "/map.bin"), minmax = read_all<double>(dir + "/minmax.bin");
        const std::vector<uint8_t> table_bytes = read_all<uint8_t>(dir + "/table.bin");
        mesh::DepthImage img;
        img.map = Grid<double>(map_dims.at(0), map_dims.at(1), 0.0);
        if (cells.size() != (size_t)map_dims[0] * map_dims[1] || table_bytes.size() != 768) throw std::runtime_error("bad map sizes");
        std::copy(cells.begin(), cells.end(), img.map.data());
        img.min_depth = minmax.at(0), img.max_depth = minmax.at(1);
        std::array<uint8_t, 768> table;
        std::copy(table_bytes.begin(), table_bytes.end(), table.begin());
        const std::vector<uint8_t> rgba = mesh::colour_map(dev, img, table);
        write_all(dir + "/rgba.bin", rgba.data(), rgba.size());
        std::printf("{\"plain\": %zu, \"color\": %zu, \"color_header\": %llu, \"color_vertices\": %llu, \"color_faces\": %llu, \"rgba\": %zu}\n",
                    plain.size(), color.size(), (unsigned long long)color_sec.header, (unsigned long long)color_sec.vertices,
                    (unsigned long long)color_sec.faces, rgba.size());
        // a mode the library does not know is refused with a message, as an exception
        try {
            mesh::ply(dev, s, polygons, {}, (mesh::VertexMode)3, out_scale);
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
