/* TEST INFRASTRUCTURE: the CPU checker of the segment tests (tests/segments_cases.py), written from the definition of unc_segment_t
 * in include/uncalled_hip.h and compiled with gcc -O2 -ffp-contract=off.  It goes over the path from its START (the last pair) to
 * its end, row by row -- not from heads found in parallel, as the kernel does -- so the two share the definition and nothing else.
 *
 * path: n_pairs pairs (column, row), end cell first, as DTW::get_path() gives them.
 * ev_*: the query's KEPT events (what the detector emitted), col_evt[c] = the event that is column c.
 * out: room for one record per row of the path.  Returns the number of rows; *row_first receives the first. */
#include <math.h>
#include <stdint.h>

typedef struct {
    uint64_t smp_st;
    uint32_t smp_span, smp_n, col_first, n_cols;
    float mean, stdv, level;
    uint32_t shared;
} seg_t;

uint32_t segments_check(const uint32_t *path, uint64_t n_pairs, const float *ev_mean, const float *ev_stdv, const uint32_t *ev_start,
                        const uint32_t *ev_length, const uint32_t *col_evt, uint64_t query_smp_st, float scale, float shift, seg_t *out,
                        uint32_t *row_first) {
    if (n_pairs == 0) return 0;
    uint32_t n = 0;
    int64_t p = (int64_t)n_pairs - 1;
    *row_first = path[2 * p + 1];
    uint32_t prev_last_col = 0;
    while (p >= 0) {
        const uint32_t row = path[2 * p + 1];
        seg_t s;
        double S = 0.0, Q = 0.0;
        uint64_t N = 0;
        uint32_t first = 1, st = 0, en = 0, last_col = 0;
        s.col_first = path[2 * p];
        s.n_cols = 0;
        for (; p >= 0 && path[2 * p + 1] == row; --p) {
            const uint32_t c = path[2 * p], e = col_evt[c];
            const double m = (double)ev_mean[e], d = (double)ev_stdv[e], l = (double)ev_length[e];
            S += m * l;
            Q += l * (d * d + m * m);
            N += ev_length[e];
            if (first) { st = ev_start[e]; first = 0; }
            en = ev_start[e] + ev_length[e];
            last_col = c;
            s.n_cols++;
        }
        const double M = S / (double)N;
        s.smp_st = query_smp_st + st;
        s.smp_span = en - st;
        s.smp_n = (uint32_t)N;
        s.mean = (float)M;
        s.stdv = (float)sqrt(fmax(Q / (double)N - M * M, 0.0));
        const float prod = scale * s.mean;
        s.level = prod + shift;
        s.shared = n > 0 && s.col_first == prev_last_col ? 1u : 0u;
        prev_last_col = last_col;
        out[n++] = s;
    }
    return n;
}
