/* TEST INFRASTRUCTURE: plain-C restatement of the stages between event detection and DTW of read-to-reference alignment -- the stall
 * mask (EventProfiler::get_full_mask, event_profiler.hpp:71-104,129-151 over Normalizer::push, normalizer.cpp:46-75), the target of
 * dtw_test.cpp:106-116 and Normalizer::set_signal / pop (normalizer.cpp:31-44,114-128).  Written from the reference's text, with a
 * ring for the window as the reference keeps one (the kernel does without).  gcc -O2 -ffp-contract=off. */
#include <math.h>
#include <stdint.h>

#define WIN 25u

/* mask[i] = 1: event i is kept.  Returns how many are. */
uint32_t align_check_mask(const float *means, uint32_t n, uint8_t *mask) {
    float ring[WIN];
    double mean = 0, varsum = 0;
    uint32_t cnt = 0, rd = 0, wr = 0, full = 0, to_mask = 0, is_full = 0, decided = 0, kept = 0;
    ring[0] = 0;
    for (uint32_t e = 0; e < n; e++) {
        float newevt = means[e];
        double oldevt = ring[wr];
        ring[wr] = newevt;
        if (cnt == WIN) {
            double oldmean = mean;
            mean += (newevt - oldevt) / WIN;
            varsum += (newevt + oldevt - oldmean - mean) * (newevt - oldevt);
        } else {
            cnt++;
            double dt1 = newevt - mean;
            mean += dt1 / cnt;
            double dt2 = newevt - mean;
            varsum += dt1 * dt2;
        }
        wr = (wr + 1) % WIN;
        full = wr == rd;
        uint32_t unread = rd < wr ? wr - rd : (cnt - rd) + wr;
        if (unread > WIN / 2) {
            float stdv = (float)sqrt(varsum / cnt);
            if (stdv < 5.0f) to_mask = WIN - 1;
            else if (to_mask > 0) to_mask--;
            if (full) {
                rd = (rd + 1) % WIN;
                full = 0;
                is_full = 1;
            }
        }
        if (is_full) {
            mask[decided] = to_mask == 0;
            kept += mask[decided++];
        }
    }
    while (decided < n) {
        if (to_mask == 0) mask[decided] = 1;
        else { mask[decided] = 0; to_mask--; }
        kept += mask[decided++];
    }
    return kept;
}

/* dtw_test.cpp:106-116 over the template model's means */
void align_check_target(const float *model_means, const uint16_t *kmers, uint64_t n, float *tgt_mean, float *tgt_stdv) {
    float read_mean = 0;
    for (uint64_t i = 0; i < n; i++) read_mean += model_means[kmers[i]];
    read_mean /= (float)n;
    float read_stdv = 0;
    for (uint64_t i = 0; i < n; i++) {
        float d = model_means[kmers[i]] - read_mean;
        read_stdv = (float)((double)read_stdv + (double)d * (double)d);
    }
    *tgt_mean = read_mean;
    *tgt_stdv = sqrtf(read_stdv / (float)n);
}

/* Normalizer(tgt_mean, tgt_stdv).set_signal(x), then pop until empty */
void align_check_normalize(const float *x, uint32_t n, float tgt_mean, float tgt_stdv, float *out, float *scale_out, float *shift_out) {
    double mean = 0, varsum = 0;
    for (uint32_t i = 0; i < n; i++) mean += x[i];
    mean /= n;
    for (uint32_t i = 0; i < n; i++) {
        double e = x[i] - mean;
        varsum += e * e;
    }
    float scale = (float)(tgt_stdv / sqrt(varsum / n));
    float shift = (float)(tgt_mean - scale * mean);
    for (uint32_t i = 0; i < n; i++) {
        float t = scale * x[i];
        out[i] = t + shift;
    }
    *scale_out = scale;
    *shift_out = shift;
}
