// host_mesh_obj: the OBJ writer through the C++ host layer (cvhip_host.hpp, namespace mesh: mesh_obj, mesh_obj_mtl).
// usage: host_mesh_obj <dir> <n> <m>   - reads <dir>/points.bin (n x 3 f64), tracks.bin (n x m x 2 i32), polygons.bin (u32
// triples), cameras.bin (u32 per polygon), images.bin (the m RGB8 images, concatenated), dims.bin (m x 2 u32: width, height) and
// scale.bin (3 f64); writes plain.obj, color.obj, scene.obj, scene.mtl and prints one JSON line.
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

static void write_all(const std::string &path, const void *data, size_t bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char *>(data), (std::streamsize)bytes);
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
        const std::vector<uint32_t> flat = read_all<uint32_t>(dir + "/polygons.bin"), cameras = read_all<uint32_t>(dir + "/cameras.bin");
        const std::vector<uint32_t> dims = read_all<uint32_t>(dir + "/dims.bin");
        const std::vector<uint8_t> pixels = read_all<uint8_t>(dir + "/images.bin");
        const std::vector<double> scale = read_all<double>(dir + "/scale.bin");
        if (flat.size() != 3 * cameras.size()) throw std::runtime_error("one camera per polygon");
        std::vector<mesh::Polygon> polygons;
        for (size_t p = 0; p < cameras.size(); p++) polygons.push_back(mesh::Polygon{cameras[p], {flat[3 * p], flat[3 * p + 1], flat[3 * p + 2]}});
        std::vector<mesh::RgbImage> images(m), sizes(m); // sizes: no pixels, which Texture mode does not read
        size_t at = 0;
        for (size_t c = 0; c < m; c++) {
            sizes[c].width = images[c].width = dims[2 * c], sizes[c].height = images[c].height = dims[2 * c + 1];
            const size_t bytes = (size_t)images[c].width * images[c].height * 3;
            images[c].pixels.assign(pixels.begin() + at, pixels.begin() + at + bytes);
            at += bytes;
        }
        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        const std::array<double, 3> out_scale{scale.at(0), scale.at(1), scale.at(2)};
        mesh::ObjSections sec;
        const std::vector<uint8_t> plain = mesh::mesh_obj(dev, s, polygons, {}, mesh::VertexMode::Plain, out_scale, "scene");
        const std::vector<uint8_t> color = mesh::mesh_obj(dev, s, polygons, images, mesh::VertexMode::Color, out_scale, "scene");
        const std::vector<uint8_t> texture = mesh::mesh_obj(dev, s, polygons, sizes, mesh::VertexMode::Texture, out_scale, "scene", &sec);
        const std::string mtl = mesh::mesh_obj_mtl("scene", (uint32_t)m);
        write_all(dir + "/plain.obj", plain.data(), plain.size());
        write_all(dir + "/color.obj", color.data(), color.size());
        write_all(dir + "/scene.obj", texture.data(), texture.size());
        write_all(dir + "/scene.mtl", mtl.data(), mtl.size());
        std::printf("{\"plain\": %zu, \"color\": %zu, \"texture\": %zu, \"sections\": [%llu, %llu, %llu, %llu]}\n", plain.size(), color.size(),
                    texture.size(), (unsigned long long)sec.header, (unsigned long long)sec.v, (unsigned long long)sec.vt,
                    (unsigned long long)sec.f);
        // a mode the library does not know is refused with a message, as an exception
        try {
            mesh::mesh_obj(dev, s, polygons, {}, (mesh::VertexMode)3, out_scale, "scene");
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
