// midaspom_amd/csrc/spom_scn_row.h -- the model of the first survey row that
// the exact scenario engine (spom_scenario_plan.cpp) and the scenario
// simulator (spom_scnsim_plan.cpp) share: one copy of the row check, the
// dispersal table, the source rows and the float priors of the completions of
// main_MIDASPOM_dieoff.c / main_MIDASPOM_loss.c, so that the two engines hold
// the same bytes.  Host only; include it from units built with
// -ffp-contract=off.
#ifndef SPOM_SCN_ROW_H
#define SPOM_SCN_ROW_H
#include <cmath>
#include <cstdint>
#include <vector>

#include "mdp_internal.h"

// every survey value is -1 (missing), 0 or 1
inline int scn_check_row(const int32_t *row, uint32_t n)
{
    for (uint32_t j = 0; j < n; ++j)
        if (row[j] < -1 || row[j] > 1) return mdp_set_error(MDP_EINVAL, "observation %d not in {-1,0,1}", row[j]);
    return MDP_OK;
}

// M[l][k] = exp(-(1/m)|l-k|d) for l != k < n, rows of ld >= n doubles
// (dieoff.c:238-248); the diagonal and the padding keep what M holds
inline void scn_dispersal(uint32_t n, double m, double d, uint32_t ld, double *M)
{
    const double a = 1.0 / m;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) M[(size_t)i * ld + j] = M[(size_t)j * ld + i] = exp(-a * (double)(j - i) * d);
}

// src[id][k] = exp(-(1/m)(k+1) dsrc[id]), k < n (loss.c:365), rows of ld >= n doubles
inline void scn_source_rows(uint32_t n, double m, const double *dsrc, uint32_t nd, uint32_t ld, double *src)
{
    for (uint32_t id = 0; id < nd; ++id)
        for (uint32_t k = 0; k < n; ++k) src[(size_t)id * ld + k] = exp(-(1.0 / m) * (k + 1) * dsrc[id]);
}

// float priors of the 2^nmiss completions (dieoff.c:205-232): completion k
// holds the q-th missing patch in bit nmiss-1-q; the factors are multiplied
// in ascending q
inline void scn_priors(uint32_t nmiss, float p, std::vector<float> *prior)
{
    const uint32_t np = 1u << nmiss;
    prior->assign(np, 1.0f);
    for (uint32_t q = 0; q < nmiss; ++q) {
        const uint32_t st1 = np >> (q + 1);
        for (uint32_t k = 0; k < np; ++k) {
            const uint32_t bitv = k / st1 % 2;
            (*prior)[k] *= (float)bitv * p + (float)(1 - bitv) * (1 - p);
        }
    }
}

#endif
