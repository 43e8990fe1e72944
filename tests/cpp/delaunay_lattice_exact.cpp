// LatticePolicy of cybervision_amd/csrc/delaunay_common.hpp (the header without HIP) against ExactPolicy, as plain C++: every
// star of a points file (k x 2 f64, integer-valued within 2^24) is built with both policies, and a star that the lattice
// policy finishes must emit the exact policy's faces, in their order.  A star that it flags (a duplicate met on the way)
// takes the exact policy's faces, as in the library.
//   delaunay_lattice_exact <points.bin> <faces.bin> [cells]  -> faces.bin (f x 3 uint32), one JSON line on stdout
// ("flagged": the stars the lattice policy left; "over": the stars that visited more than `cells` grid cells, default 1024)
// Built by tests/test_delaunay_lattice_cpu.py with -fsanitize=address,undefined: UBSan's signed-overflow check is what a
// 64-bit in-circle determinant would trip.
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
        std::fprintf(stderr, "usage: %s points.bin faces.bin [cells]\n", argv[0]);
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
    for (const double v : xy)
        if (!on_lattice(v)) {
            std::fprintf(stderr, "%.17g is not an integer within 2^24: the lattice policy does not apply\n", v);
            return 2;
        }
    const uint32_t k = (uint32_t)(xy.size() / 2);
    const uint64_t limit = argc == 4 ? std::strtoull(argv[3], nullptr, 10) : 1024;
    std::vector<uint32_t> all;
    uint64_t flagged = 0, over = 0, most_cells = 0;
    if (k) {
        std::vector<uint32_t> cell_start, cell_pts;
        const Grid g = host_grid(xy.data(), k, cell_start, cell_pts);
        Duplicates dups(g);
        const ExactPolicy exact{&dups};
        const LatticePolicy lattice;
        for (uint32_t a = 0; a < k; a++) {
            Collect want, got;
            uint64_t cells = 0, lattice_cells = 0;
            if (!build_star(g, exact, a, UINT64_MAX, k, want, &cells)) {
                std::fprintf(stderr, "star %u left the exact path\n", a);
                return 1;
            }
            if (!build_star(g, lattice, a, UINT64_MAX, k, got, &lattice_cells)) {
                flagged++;
            } else if (got.faces != want.faces) {
                std::fprintf(stderr, "star %u: the lattice policy's faces (%zu) are not the exact policy's (%zu)\n", a, got.faces.size() / 3,
                             want.faces.size() / 3);
                return 1;
            } else {
                if (lattice_cells > most_cells) most_cells = lattice_cells;
                over += lattice_cells > limit;
            }
            all.insert(all.end(), want.faces.begin(), want.faces.end());
        }
    }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) {
        std::perror(argv[2]);
        return 2;
    }
    if (!all.empty()) std::fwrite(all.data(), sizeof(uint32_t), all.size(), f);
    std::fclose(f);
    std::printf("{\"k\": %u, \"faces\": %zu, \"flagged\": %llu, \"most_cells\": %llu, \"over\": %llu}\n", k, all.size() / 3,
                (unsigned long long)flagged, (unsigned long long)most_cells, (unsigned long long)over);
    return 0;
}
