// host_tracks: the dense track table in device memory through the C++ host layer (cvhip_host.hpp, mesh::TrackTable).
// usage: host_tracks <dir> <W> <H> <m>   - reads <dir>/img1.raw and <dir>/img2.raw (W x H u8), <dir>/f.bin (9 f64) and
// <dir>/start.bin (n x m x 2 i32); correlates the pair over its box pyramid, then assign -> extend (0, 1) -> merge (image 0) ->
// gather (row j * 7919 mod rows, 500 of them).  Writes <dir>/after_extend.bin, <dir>/after_merge.bin and <dir>/gathered.bin
// (i32) and prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../cybervision_amd/csrc/host/cvhip_host.hpp"

using namespace cvhip_host;

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

static Grid<uint8_t> load_image(const std::string &path, size_t w, size_t h)
{
    const std::vector<uint8_t> px = read_all<uint8_t>(path);
    if (px.size() != w * h) throw std::runtime_error("size of " + path);
    Grid<uint8_t> g(w, h, 0);
    std::copy(px.begin(), px.end(), g.data());
    return g;
}

static Grid<uint8_t> box_downsample(const Grid<uint8_t> &s)
{
    Grid<uint8_t> d(s.width() / 2, s.height() / 2, 0);
    for (size_t y = 0; y < d.height(); y++)
        for (size_t x = 0; x < d.width(); x++) {
            const unsigned v = s.val(2 * x, 2 * y) + s.val(2 * x + 1, 2 * y) + s.val(2 * x, 2 * y + 1) + s.val(2 * x + 1, 2 * y + 1);
            d.val_mut(x, y) = (uint8_t)((v + 2) >> 2);
        }
    return d;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const std::string dir = argv[1];
    try {
        const uint32_t w = (uint32_t)std::strtoul(argv[2], nullptr, 10), h = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        const uint32_t m = (uint32_t)std::strtoul(argv[4], nullptr, 10);
        const std::vector<double> fv = read_all<double>(dir + "/f.bin");
        if (fv.size() != 9) throw std::runtime_error("f.bin holds 9 doubles");
        std::array<double, 9> f;
        std::copy(fv.begin(), fv.end(), f.begin());
        const std::vector<int32_t> start = read_all<int32_t>(dir + "/start.bin");

        GpuDevice dev = create_gpu_context(HardwareMode::Gpu);
        std::vector<Grid<uint8_t>> p1{load_image(dir + "/img1.raw", w, h)}, p2{load_image(dir + "/img2.raw", w, h)};
        const size_t steps = PointCorrelations::optimal_scale_steps({w, h});
        for (size_t i = 0; i < steps; i++) {
            p1.push_back(box_downsample(p1.back()));
            p2.push_back(box_downsample(p2.back()));
        }
        PointCorrelations pc(dev, {w, h}, {w, h}, f, ProjectionMode::Perspective);
        for (size_t i = 0; i <= steps; i++) {
            const size_t k = steps - i;
            pc.correlate_images(p1[k], p2[k], 1.0f / (float)(1u << k));
        }

        mesh::TrackTable table(dev, m);
        table.assign(start);
        const uint64_t rows_start = table.rows();
        const mesh::TrackTable::ExtendCounts ext = table.extend(pc, 0, 1, std::max(w, h));
        const uint64_t rows_extended = table.rows();
        write_all(dir + "/after_extend.bin", table.read());
        const mesh::TrackTable::MergeStats st = table.merge(0, w, h);
        const uint64_t rows_merged = table.rows();
        write_all(dir + "/after_merge.bin", table.read());
        std::vector<uint64_t> rows(rows_merged ? 500 : 0);
        for (size_t j = 0; j < rows.size(); j++) rows[j] = (uint64_t)j * 7919 % rows_merged;
        write_all(dir + "/gathered.bin", table.gather(rows));
        std::printf("{\"rows_start\": %llu, \"matched\": %llu, \"filled\": %llu, \"appended\": %llu, \"rows_extended\": %llu, "
                    "\"present\": %llu, \"cells\": %llu, \"rejected\": %llu, \"empty_area\": %llu, \"rows_merged\": %llu, \"m\": %u}\n",
                    (unsigned long long)rows_start, (unsigned long long)ext.matched, (unsigned long long)ext.filled,
                    (unsigned long long)ext.appended, (unsigned long long)rows_extended, (unsigned long long)st.present,
                    (unsigned long long)st.cells, (unsigned long long)st.rejected, (unsigned long long)st.empty_area,
                    (unsigned long long)rows_merged, table.m());
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
