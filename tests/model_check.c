/* TEST INFRASTRUCTURE: the three tables of a pore model, restated from the reference's PoreModel (pore_model.hpp: init_kmer :58-62,
 * the pair constructor :77-103, init_stdv :48-56) against the same libm as the library.  Compiled by tests/model_cases.py with
 * gcc -O2 -ffp-contract=off.  The reference's expressions, with C++'s promotions written out:
 *   lv_vars_x2_[k] = 2 * stdv * stdv                     float products, left to right
 *   lognorm_denoms_[k] = log(sqrt(M_PI * lv_vars_x2_[k]))   double, stored as float
 *   model_mean_ += mean; model_mean_ /= kmer_count_     float
 *   model_stdv_ += pow(lv_means_[kmer] - model_mean_, 2)   float difference, squared in double, added in double, stored as float
 *   model_stdv_ = sqrt(model_stdv_ / kmer_count_)        float */
#include <math.h>
#include <stdint.h>

void model_check_tables(const float *pairs2048, int cmpl, float *means, float *vars_x2, float *lognorm, float *model_mean, float *model_stdv) {
    float mm = 0.0f;
    for (uint32_t kmer = 0; kmer < 1024; ++kmer) {
        const float mean = pairs2048[2 * kmer], stdv = pairs2048[2 * kmer + 1];
        const uint32_t k = cmpl ? kmer ^ 0x3FFu : kmer;
        means[k] = mean;
        vars_x2[k] = 2 * stdv * stdv;
        lognorm[k] = (float)log(sqrt(M_PI * vars_x2[k]));
        mm += mean;
    }
    mm /= 1024;
    float sd = 0.0f;
    for (uint32_t k = 0; k < 1024; ++k) sd += pow(means[k] - mm, 2);
    *model_mean = mm;
    *model_stdv = sqrtf(sd / 1024);
}
