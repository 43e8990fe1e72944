// The exact host path of cvhip_mesh_delaunay as plain C++ (cybervision_amd/csrc/delaunay_common.hpp without HIP): every
// star of a points file (k x 2 f64) by the wrapping routine with the exact predicates and the tie rule.
//   delaunay_host_exact <points.bin> <faces.bin> [cells]  -> faces.bin (f x 3 uint32), one JSON line on stdout
// ("over": the stars that visited more than `cells` grid cells, default 1024 - what a lane_cells of that size sends to the host)
// Built by tests/test_delaunay_host_cpu.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cybervision_amd/csrc/delaunay_common.hpp"

using namespace cvhip::delaunay;

struct Collect {
    std::vector<uint32_t> faces;
    void operator()(uint32_t a, uint32_t b, uint32_t c)
    {
        if (a < b && a < c) faces.insert(faces.end(), {a, b, c});
    }
};

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: %s points.bin faces.bin\n", argv[0]);
        return 2;
    }
    std::vector<double> xy;
    if (FILE *f = std::fopen(argv[1], "rb")) {
        double buf[2];
        while (std::fread(buf, sizeof(double), 2, f) == 2) xy.insert(xy.end(), buf, buf + 2);
        std::fclose(f);
    } else {
        std::perror(argv[1]);
        return 2;
    }
    const uint32_t k = (uint32_t)(xy.size() / 2);
    Collect out;
    const uint64_t limit = argc == 4 ? std::strtoull(argv[3], nullptr, 10) : 1024;
    uint64_t duplicates = 0, most_cells = 0, over = 0, all_cells = 0;
    if (k) {
        std::vector<uint32_t> cell_start, cell_pts;
        const Grid g = host_grid(xy.data(), k, cell_start, cell_pts);
        Duplicates dups(g);
        const ExactPolicy pol{&dups};
        for (uint32_t a = 0; a < k; a++) {
            uint64_t cells = 0;
            if (!build_star(g, pol, a, UINT64_MAX, k, out, &cells)) {
                std::fprintf(stderr, "star %u left the exact path\n", a);
                return 1;
            }
            if (cells > most_cells) most_cells = cells;
            over += cells > limit, all_cells += cells;
        }
        duplicates = dups.count_all();
    }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) {
        std::perror(argv[2]);
        return 2;
    }
    if (!out.faces.empty()) std::fwrite(out.faces.data(), sizeof(uint32_t), out.faces.size(), f);
    std::fclose(f);
    std::printf("{\"k\": %u, \"faces\": %zu, \"duplicates\": %llu, \"most_cells\": %llu, \"over\": %llu, \"cells\": %llu}\n", k,
                out.faces.size() / 3, (unsigned long long)duplicates, (unsigned long long)most_cells, (unsigned long long)over,
                (unsigned long long)all_cells);
    return 0;
}
