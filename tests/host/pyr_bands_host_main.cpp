// Prints k_pyr_rows' band descriptors (PyrBand, coeb-slam_amd/csrc/coeb_plan.hpp) of the plan of a
// W x H image (1000 features; default 8 levels at scale 1.2), for tests/test_pyr_bands_host.py,
// which recomputes them in numpy.  Usage: pyr_bands_host W H [nlevels [scale]]
//   patterns <n> <mask>...
//   level <l> <sw> <sh> <sp> <dw> <dh> <pitch> <rows_ok> <nbands>
//   band <pattern> <src_off> <dst_off> <pad> <beta0> ... <beta7>       (nbands lines per level)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "coeb_plan.hpp"

int main(int argc, char** argv)
{
    if (argc < 3 || argc > 5) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    coeb_orb_params p;
    memset(&p, 0, sizeof p);
    p.nfeatures = 1000; p.scale_factor = argc > 4 ? (float)atof(argv[4]) : 1.2f; p.nlevels = argc > 3 ? atoi(argv[3]) : 8;
    p.ini_th_fast = 20; p.min_th_fast = 7;
    Tables t;
    Plan P;
    std::vector<int> rtab;
    std::vector<CellDesc> cells;
    std::string err;
    if (!make_tables(p, t) || !make_plan(t, W, H, 0, P, rtab, cells, err)) {
        fprintf(stderr, "no plan: %s\n", err.c_str());
        return 1;
    }
    printf("patterns %d", kPyrPatterns);
    for (int i = 0; i < kPyrPatterns; i++) printf(" %u", kPyrPatternMask[i]);
    printf("\n");
    for (int l = 1; l < P.L; l++) {
        const LevelGeom& g = P.lv[l];
        const LevelGeom& s = P.lv[l - 1];
        const int nbands = (g.h + kPyrBandRows - 1) / kPyrBandRows;
        if (g.band_off % 4 != 0 || (size_t)g.band_off + (size_t)nbands * kPyrBandInts > rtab.size()) {
            fprintf(stderr, "level %d: band table outside the resize table\n", l);
            return 1;
        }
        printf("level %d %d %d %d %d %d %d %d %d\n", l, s.w, s.h, s.pitch, g.w, g.h, g.pitch, g.rows_ok, nbands);
        for (int b = 0; b < nbands; b++) {
            printf("band");
            for (int k = 0; k < kPyrBandInts; k++) printf(" %d", rtab[(size_t)g.band_off + (size_t)b * kPyrBandInts + k]);
            printf("\n");
        }
    }
    return 0;
}
