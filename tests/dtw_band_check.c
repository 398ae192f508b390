/* TEST INFRASTRUCTURE: a plain restatement of banded global DTW as include/uncalled_hip.h defines it (unc_dtw_band_batch), the
 * yardstick of tests/test_dtw_band_cpu.py and tests/test_gpu_dtw_band.py (tests/dtw_band_check.py compiles it at test time with
 * -ffp-contract=off).  Column-major sweep: column j holds rows c(j) - W .. c(j) + W, two columns of scores, one byte of
 * back-pointer per band cell: O(cols * (2 W + 1)) memory, so it takes long alignments. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { MV_D = 0, MV_H = 1, MV_V = 2 };
enum { ST_OK = 0, ST_TOO_NARROW = 5, ST_LEFT_BAND = 6 };

static float band_cost(uint32_t cost, const float *model, uint32_t k, float e) {
    const float d = e - model[k];
    if (cost == 1) return fabsf(d);
    const double q = -((double)d * (double)d) / (double)model[1024 + k] - (double)model[2048 + k];
    return -(float)q;
}

static uint64_t centre(uint64_t j, uint64_t rows, uint64_t cols) { return j * rows / cols; }
static int in_band(int64_t i, uint64_t j, uint64_t rows, uint64_t cols, uint64_t W) {
    const uint64_t c = centre(j, rows, cols);
    return i >= 0 && (uint64_t)i + W >= c && (uint64_t)i <= c + W;
}

/* path: room for rows + cols - 1 pairs (event j, k-mer i), end cell first.  Returns 0, or -1 without memory.
 * status: 0, 5 (the band holds no path to the last cell: nothing computed, score 0, path_len 0) or 6 (the traceback stopped at the
 * last cell inside the band: path_len counts the pairs up to it).  ties: band cells whose smallest move is not alone. */
int dtw_band_check(const float *ev, uint64_t cols, const uint16_t *km, uint64_t rows, const float *model, uint32_t cost, float dw,
                   float hw, float vw, uint64_t band, float *score, uint64_t *path_len, uint32_t *path, uint32_t *status, uint64_t *ties) {
    const float MAXC = FLT_MAX / 2.0f;
    *score = 0; *path_len = 0; *status = ST_OK;
    if (ties) *ties = 0;
    if ((rows + cols - 1) / cols > band + 1) { *status = ST_TOO_NARROW; return 0; }
    /* (at W >= rows every cell is in the band: the membership test is the same with W = rows, and the storage stays bounded) */
    const uint64_t W = band < rows ? band : rows, H = 2 * W + 1;
    uint8_t *mv = malloc(cols * H);
    float *prev = malloc(H * sizeof(float)), *cur = malloc(H * sizeof(float));
    if (!mv || !prev || !cur) { free(mv); free(prev); free(cur); return -1; }
    uint64_t n_ties = 0;
    /* slot of row i in column j: i - (c(j) - W) = i + W - c(j), in [0, 2 W] */
    uint64_t cprev = 0;
    for (uint64_t j = 0; j < cols; ++j) {
        const uint64_t c = centre(j, rows, cols);
        const uint64_t ilo = c > W ? c - W : 0, ihi = c + W < rows - 1 ? c + W : rows - 1;
        for (uint64_t i = ilo; i <= ihi; ++i) {
            const float x = band_cost(cost, model, km[i], ev[j]);
            float d, h, v;
            if (i > 0 && j > 0) d = in_band((int64_t)i - 1, j - 1, rows, cols, W) ? prev[i - 1 + W - cprev] : MAXC;
            else d = i == j ? 0 : MAXC;
            if (j > 0) h = in_band((int64_t)i, j - 1, rows, cols, W) ? prev[i + W - cprev] : MAXC;
            else h = MAXC;
            if (i > 0) v = i - 1 >= ilo ? cur[i - 1 + W - c] : MAXC;
            else v = MAXC;
            const float ds = d + dw * x, hs = h + hw * x, vs = v + vw * x;
            float m;
            uint8_t w;
            if (ds <= hs && ds <= vs) { m = ds; w = MV_D; n_ties += ds == hs || ds == vs; }
            else if (hs <= vs) { m = hs; w = MV_H; n_ties += hs == vs; }
            else { m = vs; w = MV_V; }
            cur[i + W - c] = m;
            mv[j * H + (i + W - c)] = w;
        }
        float *t = prev; prev = cur; cur = t;
        cprev = c;
    }
    /* prev holds the last column; (rows - 1, cols - 1) is in the band by the feasibility test */
    uint64_t i = rows - 1, j = cols - 1;
    *score = prev[i + W - cprev];
    uint64_t n = 0;
    for (;;) {
        if (!in_band((int64_t)i, j, rows, cols, W)) { *status = ST_LEFT_BAND; break; }
        path[2 * n] = (uint32_t)j; path[2 * n + 1] = (uint32_t)i; ++n;
        if (i == 0 && j == 0) break;
        const uint8_t w = mv[j * H + (i + W - centre(j, rows, cols))];
        if (i == 0 || (w == MV_H && j > 0)) --j;
        else if (j == 0 || w == MV_V) --i;
        else { --i; --j; }
    }
    *path_len = n;
    if (ties) *ties = n_ties;
    free(mv); free(prev); free(cur);
    return 0;
}
