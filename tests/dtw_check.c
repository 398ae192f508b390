/* TEST INFRASTRUCTURE: a plain restatement of full-matrix DTW with the two r9.4 costs, the yardstick for alignments too large for
 * the committed goldens (tests/dtw_check.py compiles it at test time with -ffp-contract=off; it reproduces every golden bit for bit).
 * Row-major sweep, two rows of scores, one byte of back-pointer per cell. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { SUB_NONE = 0, SUB_ROW = 1, SUB_COL = 2 };
enum { MV_D = 0, MV_H = 1, MV_V = 2 };

float dtw_check_cost(uint32_t cost, const float *model, uint32_t k, float e) {
    const float d = e - model[k];
    if (cost == 1) return fabsf(d);
    const double q = -((double)d * (double)d) / (double)model[1024 + k] - (double)model[2048 + k];
    return -(float)q;
}

/* path: room for rows + cols - 1 pairs (event j, k-mer i), end cell first.  end_min_cells, last_is_min (either may be null): how
 * many cells of the line the end-cell search scans (ROW: the last column, COL: the last row; NONE scans nothing: 0) equal its
 * smallest value, and whether the matrix's last cell is one of them -- the premise of the tests of ties at the end cell.
 * Returns 0, or -1 without memory. */
int dtw_check(const float *ev, uint64_t cols, const uint16_t *km, uint64_t rows, const float *model, uint32_t subseq, uint32_t cost,
              float dw, float hw, float vw, float *score, uint64_t *path_len, uint32_t *path, uint64_t *ties, uint64_t *end_min_cells,
              uint32_t *last_is_min) {
    const float MAXC = FLT_MAX / 2.0f;
    uint8_t *mv = malloc(rows * cols);
    float *prev = malloc(cols * sizeof(float)), *cur = malloc(cols * sizeof(float)), *lastcol = malloc(rows * sizeof(float));
    if (!mv || !prev || !cur || !lastcol) { free(mv); free(prev); free(cur); free(lastcol); return -1; }
    uint64_t n_ties = 0;
    for (uint64_t i = 0; i < rows; ++i) {
        for (uint64_t j = 0; j < cols; ++j) {
            const float c = dtw_check_cost(cost, model, km[i], ev[j]);
            float d, h, v;
            if (i > 0 && j > 0) d = prev[j - 1];
            else if (i == j || (i == 0 && subseq == SUB_COL) || (j == 0 && subseq == SUB_ROW)) d = 0;
            else d = MAXC;
            if (j > 0) h = cur[j - 1]; else h = subseq == SUB_ROW ? 0 : MAXC;
            if (i > 0) v = prev[j]; else v = subseq == SUB_COL ? 0 : MAXC;
            const float ds = d + dw * c, hs = h + hw * c, vs = v + vw * c;
            float m;
            uint8_t w;
            if (ds <= hs && ds <= vs) { m = ds; w = MV_D; n_ties += ds == hs || ds == vs; }
            else if (hs <= vs) { m = hs; w = MV_H; n_ties += hs == vs; }
            else { m = vs; w = MV_V; }
            cur[j] = m;
            mv[i * cols + j] = w;
        }
        lastcol[i] = cur[cols - 1];
        float *t = prev; prev = cur; cur = t;
    }
    /* prev now holds the last row */
    uint64_t i = rows - 1, j = cols - 1;
    if (subseq == SUB_ROW) { for (uint64_t k = 0; k < rows; ++k) if (lastcol[k] < lastcol[i]) i = k; *score = lastcol[i]; }
    else if (subseq == SUB_COL) { for (uint64_t k = 0; k < cols; ++k) if (prev[k] < prev[j]) j = k; *score = prev[j]; }
    else *score = prev[j];
    {   /* (a NaN is neither the minimum nor equal to it) */
        const float *scan = subseq == SUB_ROW ? lastcol : prev;
        const uint64_t n_scan = subseq == SUB_ROW ? rows : subseq == SUB_COL ? cols : 0;
        float mn = 0;
        uint64_t n_min = 0;
        for (uint64_t k = 0; k < n_scan; ++k) {
            if (scan[k] != scan[k]) continue;
            if (n_min == 0 || scan[k] < mn) { mn = scan[k]; n_min = 1; }
            else if (scan[k] == mn) ++n_min;
        }
        if (end_min_cells) *end_min_cells = n_min;
        if (last_is_min) *last_is_min = n_scan > 0 && n_min > 0 && scan[n_scan - 1] == mn;
    }
    uint64_t n = 0;
    path[2 * n] = (uint32_t)j; path[2 * n + 1] = (uint32_t)i; ++n;
    while (!((i == 0 || subseq == SUB_ROW) && (j == 0 || subseq == SUB_COL))) {
        const uint8_t w = mv[i * cols + j];
        if (i == 0 || w == MV_H) --j;
        else if (j == 0 || w == MV_V) --i;
        else { --i; --j; }
        path[2 * n] = (uint32_t)j; path[2 * n + 1] = (uint32_t)i; ++n;
    }
    *path_len = n;
    if (ties) *ties = n_ties;
    free(mv); free(prev); free(cur); free(lastcol);
    return 0;
}
