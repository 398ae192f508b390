/* TEST INFRASTRUCTURE: a plain restatement of the adaptive-band DTW with an open end as include/uncalled_hip.h defines it
 * (unc_dtw_adapt_batch), and of the full-matrix DTW with the same open end: the yardsticks of tests/test_dtw_adapt_cpu.py and
 * tests/test_gpu_dtw_adapt.py (tests/dtw_adapt_check.py compiles this file at test time with -ffp-contract=off).  One cell at a
 * time; a cell of anti-diagonal d lies at index i - lo_d of its anti-diagonal. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { MV_D = 0, MV_H = 1, MV_V = 2 };
enum { ST_OK = 0, ST_LEFT_BAND = 6, ST_REF_END = 7 };
#define MAXC (FLT_MAX / 2.0f)

static float cell_cost(uint32_t cost, const float *model, uint32_t k, float e) {
    const float d = e - model[k];
    if (cost == 1) return fabsf(d);
    const double q = -((double)d * (double)d) / (double)model[1024 + k] - (double)model[2048 + k];
    return -(float)q;
}

/* one cell of the recurrence (dtw.hpp:57-71) */
static float cell(float d, float h, float v, float x, float dw, float hw, float vw, uint8_t *mv) {
    const float ds = d + dw * x, hs = h + hw * x, vs = v + vw * x;
    if (ds <= hs && ds <= vs) { *mv = MV_D; return ds; }
    if (hs <= vs) { *mv = MV_H; return hs; }
    *mv = MV_V;
    return vs;
}

typedef struct {
    int64_t rows, cols, B, n_done;
    const int32_t *lo;
} band_t;

/* was (i, d - i) computed? */
static int computed(const band_t *b, int64_t d, int64_t i) {
    if (d < 0 || d >= b->n_done) return 0;
    const int64_t j = d - i;
    if (i < 0 || i >= b->rows || j < 0 || j >= b->cols) return 0;
    return i >= b->lo[d] && i < (int64_t)b->lo[d] + b->B;
}

/* path: room for rows + cols - 1 pairs (event j, k-mer i), end cell first.  lo (may be NULL): room for rows + cols - 1 values, lo_d
 * of the anti-diagonals computed; n_done: how many were.  cells (may be NULL): room for (rows + cols - 1) * B scores, cell (i, d - i)
 * at d * B + i - lo_d, NaN-free only where computed (others are left untouched).  Returns 0, or -1 without memory. */
int dtw_adapt_check(const float *ev, uint64_t cols_, const uint16_t *km, uint64_t rows_, const float *model, uint32_t cost, float dw,
                    float hw, float vw, uint64_t B_, float *score, uint64_t *path_len, uint32_t *path, uint32_t *status, int32_t *lo_out,
                    uint64_t *n_done_out, float *cells, uint32_t *end_row) {
    const int64_t rows = (int64_t)rows_, cols = (int64_t)cols_, B = (int64_t)B_, n_diag = rows + cols - 1;
    *score = 0; *path_len = 0; *status = ST_OK; *end_row = 0xFFFFFFFFu;
    int32_t *lo = malloc((size_t)n_diag * sizeof(int32_t));
    uint8_t *mv = malloc((size_t)n_diag * (size_t)B);
    float *s3 = malloc(3 * (size_t)B * sizeof(float));
    if (!lo || !mv || !s3) { free(lo); free(mv); free(s3); return -1; }
    band_t b = {rows, cols, B, 0, lo};
    int have_best = 0, have_last = 0;
    float best = INFINITY, last = 0;
    int64_t best_i = 0, last_i = 0;
    int64_t cur_lo = -B / 2;
    for (int64_t d = 0; d < n_diag; ++d) {
        int64_t it = cur_lo > 0 ? cur_lo : 0, ib = cur_lo + B - 1;
        if (d - (cols - 1) > it) it = d - (cols - 1);
        if (rows - 1 < ib) ib = rows - 1;
        if (d < ib) ib = d;
        if (it > ib) break;
        lo[d] = (int32_t)cur_lo;
        float *sd = s3 + (d % 3) * B, *s1 = s3 + ((d + 2) % 3) * B, *s2 = s3 + ((d + 1) % 3) * B;
        b.n_done = d;       /* (the predecessors lie on d - 1 and d - 2) */
        for (int64_t i = it; i <= ib; ++i) {
            const int64_t j = d - i;
            float pd, ph, pv;
            if (i == 0 && j == 0) pd = 0;
            else pd = computed(&b, d - 2, i - 1) && j >= 1 ? s2[i - 1 - lo[d - 2]] : MAXC;
            ph = j >= 1 && computed(&b, d - 1, i) ? s1[i - lo[d - 1]] : MAXC;
            pv = i >= 1 && computed(&b, d - 1, i - 1) ? s1[i - 1 - lo[d - 1]] : MAXC;
            const float x = cell_cost(cost, model, km[i], ev[j]);
            const float m = cell(pd, ph, pv, x, dw, hw, vw, &mv[d * B + (i - cur_lo)]);
            sd[i - cur_lo] = m;
            if (cells) cells[d * B + (i - cur_lo)] = m;
            if (j == cols - 1) {
                have_last = 1; last = m; last_i = i;
                if (m < best) { have_best = 1; best = m; best_i = i; }
            }
        }
        b.n_done = d + 1;
        const float st = sd[it - cur_lo], sb = sd[ib - cur_lo];
        int down;
        if (sb < st) down = 1;
        else if (st < sb) down = 0;
        else down = (int)(d & 1);
        if (cur_lo + B - 1 >= rows - 1) down = 0;       /* the band holds the last row already */
        cur_lo += down;
    }
    if (n_done_out) *n_done_out = (uint64_t)b.n_done;
    if (lo_out) for (int64_t d = 0; d < b.n_done; ++d) lo_out[d] = lo[d];
    if (!have_last) { *status = ST_LEFT_BAND; free(lo); free(mv); free(s3); return 0; }
    int64_t i = have_best ? best_i : last_i, j = cols - 1;
    *score = have_best ? best : last;
    *end_row = (uint32_t)i;
    const int at_end = i == rows - 1;
    uint64_t n = 0;
    for (;;) {
        if (!computed(&b, i + j, i)) { *status = ST_LEFT_BAND; break; }
        path[2 * n] = (uint32_t)j; path[2 * n + 1] = (uint32_t)i; ++n;
        if (i == 0 && j == 0) break;
        const uint8_t w = mv[(i + j) * B + (i - lo[i + j])];
        if (i == 0 || (w == MV_H && j > 0)) --j;
        else if (j == 0 || w == MV_V) --i;
        else { --i; --j; }
    }
    *path_len = n;
    if (*status == ST_OK && at_end) *status = ST_REF_END;
    free(lo); free(mv); free(s3);
    return 0;
}

/* the full matrix with the same recurrence and the same end scan.  cells (may be NULL): rows * cols scores, (i, j) at i * cols + j */
int dtw_open_check(const float *ev, uint64_t cols, const uint16_t *km, uint64_t rows, const float *model, uint32_t cost, float dw, float hw,
                   float vw, float *score, uint64_t *path_len, uint32_t *path, uint32_t *end_row, float *cells) {
    uint8_t *mv = malloc(rows * cols);
    float *prev = malloc(cols * sizeof(float)), *cur = malloc(cols * sizeof(float));
    if (!mv || !prev || !cur) { free(mv); free(prev); free(cur); return -1; }
    int have_best = 0;
    float best = INFINITY, last = 0;
    uint64_t best_i = 0;
    for (uint64_t i = 0; i < rows; ++i) {
        for (uint64_t j = 0; j < cols; ++j) {
            float pd, ph, pv;
            if (i == 0 && j == 0) pd = 0;
            else pd = i > 0 && j > 0 ? prev[j - 1] : MAXC;
            ph = j > 0 ? cur[j - 1] : MAXC;
            pv = i > 0 ? prev[j] : MAXC;
            const float x = cell_cost(cost, model, km[i], ev[j]);
            cur[j] = cell(pd, ph, pv, x, dw, hw, vw, &mv[i * cols + j]);
            if (cells) cells[i * cols + j] = cur[j];
        }
        last = cur[cols - 1];
        if (last < best) { have_best = 1; best = last; best_i = i; }
        float *t = prev; prev = cur; cur = t;
    }
    uint64_t i = have_best ? best_i : rows - 1, j = cols - 1;
    *score = have_best ? best : last;
    *end_row = (uint32_t)i;
    uint64_t n = 0;
    for (;;) {
        path[2 * n] = (uint32_t)j; path[2 * n + 1] = (uint32_t)i; ++n;
        if (i == 0 && j == 0) break;
        const uint8_t w = mv[i * cols + j];
        if (i == 0 || (w == MV_H && j > 0)) --j;
        else if (j == 0 || w == MV_V) --i;
        else { --i; --j; }
    }
    *path_len = n;
    free(mv); free(prev); free(cur);
    return 0;
}
