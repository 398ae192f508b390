// TEST INFRASTRUCTURE: the host side of repeat masking (uncalled_amd/csrc/unc_mask.cpp, with k_mask.hip behind it) as a stand-alone
// program for the address and undefined-behaviour sanitizers, compiled for the CPU against tests/lanesim (tests/test_mask_cpu.py builds
// and runs it).  The three functions unc_mask.cpp takes from unc_host.cpp are stood in for here, so that nothing else is linked.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "unc_dev_types.h"
#include "unc_host_util.h"

static char g_err[512];
int unc::fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
static unc::DevIndex g_ix;
int unc::index_device(const unc_index_t *) { return 0; }
const unc::DevIndex &unc::index_dev(const unc_index_t *) { return g_ix; }

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_err); return 1; } \
    } while (0)

int main() {
    unc_mask_t *m = nullptr;
    const uint8_t codes[8] = {0, 1, 2, 3, 9, 0, 1, 2};
    const uint64_t good[3] = {0, 5, 8}, desc[4] = {0, 5, 3, 8}, shortoff[2] = {0, 7}, late[2] = {1, 8};
    EXPECT(unc_mask_create(0, codes, 8, good, 2, nullptr) == UNC_ERR_ARG);
    EXPECT(unc_mask_create(0, nullptr, 8, good, 2, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(0, codes, 8, nullptr, 2, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(-1, codes, 8, good, 2, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(0, codes, 8, desc, 3, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(0, codes, 8, shortoff, 1, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(0, codes, 8, late, 1, &m) == UNC_ERR_ARG && !m);
    EXPECT(unc_mask_create(0, codes, 1ull << 32, good, 2, &m) == UNC_ERR_ARG && !m && strstr(g_err, "2^32"));
    EXPECT(lanesim_live_allocs == 0);

    // an empty masker: every call is legal and touches nothing
    const uint64_t none[2] = {0, 0};
    EXPECT(unc_mask_create(0, nullptr, 0, none, 1, &m) == UNC_OK && m);
    uint32_t km[4], occ[4], bases[4], done = 7;
    EXPECT(unc_mask_internal(m, 3, 4, km, occ, bases, &done) == UNC_OK && done == 0);
    uint64_t masked = 7;
    EXPECT(unc_mask_external(m, reinterpret_cast<const unc_index_t *>(&g_ix), 50, 1, nullptr, &masked) == UNC_OK && masked == 0);
    EXPECT(unc_mask_codes(m, nullptr) == UNC_OK);
    unc_mask_free(m);
    EXPECT(lanesim_live_allocs == 0);

    EXPECT(unc_mask_create(0, codes, 8, good, 2, &m) == UNC_OK && m);
    std::vector<uint32_t> counts(16);
    EXPECT(unc_mask_kmer_counts(nullptr, 2, counts.data()) == UNC_ERR_ARG && unc_mask_kmer_counts(m, 2, nullptr) == UNC_ERR_ARG);
    EXPECT(unc_mask_kmer_counts(m, 0, counts.data()) == UNC_ERR_ARG && unc_mask_kmer_counts(m, 14, counts.data()) == UNC_ERR_ARG);
    EXPECT(unc_mask_internal(m, 0, 1, km, occ, bases, &done) == UNC_ERR_ARG && unc_mask_internal(m, 14, 1, km, occ, bases, &done) == UNC_ERR_ARG);
    EXPECT(unc_mask_internal(m, 2, 0, km, occ, bases, &done) == UNC_ERR_ARG && unc_mask_internal(m, 2, 1, km, occ, bases, nullptr) == UNC_ERR_ARG);
    EXPECT(unc_mask_external(m, nullptr, 50, 1, nullptr, &masked) == UNC_ERR_ARG);
    const unc_index_t *ix = reinterpret_cast<const unc_index_t *>(&g_ix);
    EXPECT(unc_mask_external(m, ix, 1, 1, nullptr, &masked) == UNC_ERR_ARG && unc_mask_external(m, ix, 65536, 1, nullptr, &masked) == UNC_ERR_ARG);
    EXPECT(unc_mask_external(m, ix, 50, 0, nullptr, &masked) == UNC_ERR_ARG && unc_mask_external(m, ix, 50, 1, nullptr, nullptr) == UNC_ERR_ARG);
    float a, b, c;
    EXPECT(unc_mask_last_timing(nullptr, &b, &c) == UNC_ERR_ARG && unc_mask_last_timing(&a, &b, &c) == UNC_OK);
    // the text as uploaded: the code 9 reads as 4
    uint8_t back[8];
    EXPECT(unc_mask_codes(m, back) == UNC_OK && back[4] == 4 && back[7] == 2);
    // contigs ACGT. | ACG: AC twice, CG twice, GT once, nothing across the 4 or the contig's end
    EXPECT(unc_mask_kmer_counts(m, 2, counts.data()) == UNC_OK);
    EXPECT(counts[1] == 2 && counts[6] == 2 && counts[11] == 1 && counts[1] + counts[6] + counts[11] == 5);
    // AC and CG tie: AC goes, and with it both CG; GT is left once: one iteration of four is done
    EXPECT(unc_mask_internal(m, 2, 4, km, occ, bases, &done) == UNC_OK && done == 1);
    EXPECT(km[0] == 1 && occ[0] == 2 && bases[0] == 4);
    EXPECT(unc_mask_codes(m, back) == UNC_OK && back[0] == 4 && back[1] == 4 && back[2] == 2 && back[5] == 4 && back[7] == 2);
    unc_mask_free(m);
    EXPECT(lanesim_live_allocs == 0);
    printf("mask_host_check OK\n");
    return 0;
}
