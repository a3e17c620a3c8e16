// midaspom_amd/csrc/scnsim_plan_check.cpp -- the scenario simulator's host
// planner (spom_scnsim_plan.cpp) over one survey row, without a device or
// the HIP runtime:
//   scnsim_plan_check ROW M P D KIND "OPTIONS" NK NREP DSRC
// ROW is one character per patch: '0' empty, '1' occupied, 'm' missing.
// Prints the kernel the options select, the row's masks, FNV-1a digests of
// the missing-patch list, the dispersal table, the float priors and the source
// row at distance DSRC, and the launches of a call over NK grid points (one
// e, one c, one distance) and NREP replicates with both tables requested.
// With k_scnsim_wave<NP> selected (MDP_SIM_WAVE) the row's per-lane words and
// (lane, bit) list are printed in full, the digests are of the distance image,
// the priors and the source row, and every 16-byte slot the kernel can address
// -- every survivor l < n, every lane, every j < NP -- is checked to lie
// inside the image and to hold M's bits.
// Exit 0, or mdp_last_error() on stderr and exit 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spom_future_plan.h"  // fut_wide_slot0
#include "spom_scnsim_plan.h"

namespace {

uint64_t fnv(const void *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bit
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 10) {
        fprintf(stderr, "usage: scnsim_plan_check ROW M P D KIND \"OPTIONS\" NK NREP DSRC\n");
        return 2;
    }
    auto fail = []() {
        fprintf(stderr, "scnsim_plan_check: %s\n", mdp_last_error());
        return 1;
    };
    const uint32_t n = (uint32_t)strlen(argv[1]);
    std::vector<int32_t> row(n);
    for (uint32_t k = 0; k < n; ++k) row[k] = argv[1][k] == 'm' ? -1 : argv[1][k] - '0';
    const double m = atof(argv[2]), d = atof(argv[4]), ds = atof(argv[9]);
    const float p = (float)atof(argv[3]);
    const int kind = atoi(argv[5]);
    const uint32_t nK = (uint32_t)strtoul(argv[7], nullptr, 10);
    const uint64_t nrep = strtoull(argv[8], nullptr, 10);
    SimOpts opts;
    if (sim_parse_opts(argv[6], &opts)) return fail();
    SimPlan pl;
    if (sim_plan(row.data(), n, m, p, d, kind, opts, &pl)) return fail();
    std::vector<double> src;
    sim_src(pl, &ds, 1, &src);
    if (pl.np) {
        printf("kernel k_scnsim_wave<%u>\n", pl.np);
        printf("row n %u nmiss %u len %u\n", pl.n, pl.nmiss, pl.wlen);
        printf("fixed");
        for (uint32_t v : pl.wfixed) printf(" %x", v);
        printf("\nmissing");
        for (uint32_t v : pl.wmissmask) printf(" %x", v);
        printf("\nmiss");
        for (uint32_t v : pl.wmiss) printf(" %x", v);
        printf("\nimage %016llx prior %016llx src %016llx\n",
               (unsigned long long)fnv(pl.image.data(), pl.image.size() * sizeof(double)),
               (unsigned long long)fnv(pl.prior.data(), pl.prior.size() * sizeof(float)),
               (unsigned long long)fnv(src.data(), src.size() * sizeof(double)));
        if (src.size() != (size_t)128 * pl.np || pl.image.size() != (size_t)2 * pl.wlen || (pl.wlen & 1u)) {
            fprintf(stderr, "scnsim_plan_check: table sizes\n");
            return 1;
        }
        // every slot a lane reads for every survivor l: inside the image, and
        // the bits of the lane kernels' table entry exp(-(1/m)|l-k|d)
        const double a = 1.0 / m;
        for (uint32_t l = 0; l < n; ++l) {
            const uint32_t s0 = fut_wide_slot0(n, pl.wlen, l);
            for (uint32_t pair = 0; pair < 64 * pl.np; ++pair) {
                const size_t at = 2 * ((size_t)pair + s0);
                if (at + 1 >= pl.image.size()) {
                    fprintf(stderr, "scnsim_plan_check: slot of pair %u, survivor %u outside the image\n", pair, l);
                    return 1;
                }
                for (uint32_t q = 0; q < 2; ++q) {
                    const uint32_t k = 2 * pair + q;
                    if (k >= n) continue;  // a padded patch: never live, its sum is not used
                    const double want = k == l ? 0.0 : exp(-a * (double)(k > l ? k - l : l - k) * d);
                    if (memcmp(&want, &pl.image[at + q], sizeof want)) {
                        fprintf(stderr, "scnsim_plan_check: image entry of M[%u][%u] differs\n", l, k);
                        return 1;
                    }
                }
            }
        }
        printf("slots %u x %u inside the image\n", n, 64 * pl.np);
    } else {
        printf("kernel k_scnsim<%u>\n", pl.nm);
        printf("row n %u nmiss %u live %llx fixed %llx missing %llx\n", pl.n, pl.nmiss, (unsigned long long)pl.live,
               (unsigned long long)pl.fixed, (unsigned long long)pl.missmask);
        printf("miss %016llx M %016llx prior %016llx src %016llx\n",
               (unsigned long long)fnv(pl.miss.data(), pl.miss.size() * sizeof(uint32_t)),
               (unsigned long long)fnv(pl.M.data(), pl.M.size() * sizeof(double)),
               (unsigned long long)fnv(pl.prior.data(), pl.prior.size() * sizeof(float)),
               (unsigned long long)fnv(src.data(), src.size() * sizeof(double)));
    }
    const double e = 0.5, c = 0.5;
    std::vector<double> K(nK, 1.0);
    SimCall call;
    if (sim_call(pl, 1, 1, &e, 1, &c, 1, K.data(), nK, &ds, 1, nrep, true, pl.nmiss <= kSimMaxMatchMissing, &call))
        return fail();
    printf("call points %llu tiles_per_point %llu hist %llu match %llu launches %zu\n", (unsigned long long)call.G,
           (unsigned long long)call.tiles_per_point, (unsigned long long)call.hist_cells,
           (unsigned long long)call.match_cells, call.launches.size());
    for (const SimLaunch &l : call.launches)
        printf("launch p0 %llu npts %llu tiles %llu nwg %u\n", (unsigned long long)l.p0, (unsigned long long)l.npts,
               (unsigned long long)l.tiles, l.nwg);
    // the estimate of a table with one replicate in every completion: 2^n * sum(prior) / nrep
    if (nrep && pl.nmiss <= kSimMaxMatchMissing) {
        std::vector<uint64_t> match((size_t)1 << pl.nmiss, 1);
        double L = 0;
        if (sim_lik(pl, match.data(), 1, nrep, &L)) return fail();
        printf("lik %a\n", L);
    }
    return 0;
}
