// The pore model object (include/uncalled_hip.h: unc_model_*): the file format of PoreModel (pore_model.hpp:108-160) and the tables
// through the one builder (unc_model.h).  Host code without a kernel behind it.  Compiled as part of unc_host.cpp, which includes
// this file: every build of the library holds it, the ones without the alignment sources too (the host module loads models).
#include <hip/hip_runtime.h>

#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "unc_host_util.h"
#include "unc_model.h"

using namespace unc;

// ------------------------------------------------------------------ the model
static int model_make(const float *pairs, const char *who, unc_model_t **out) {
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER; ++k) {
        const float mean = pairs[2 * k], stdv = pairs[2 * k + 1];
        if (!std::isfinite(mean) || !std::isfinite(stdv)) return fail(UNC_ERR_ARG, "%s: k-mer %u: mean %g, stdv %g: not finite", who, k, mean, stdv);
        if (!(stdv > 0)) return fail(UNC_ERR_ARG, "%s: k-mer %u: stdv %g is not above 0", who, k, stdv);
    }
    unc_model *m = new unc_model();
    memcpy(m->pairs, pairs, sizeof m->pairs);
    model_build_tables(m->pairs, false, &m->fwd);
    *out = m;
    return UNC_OK;
}

extern "C" int unc_model_default(unc_model_t **out) {
    if (!out) return fail(UNC_ERR_ARG, "unc_model_default: null argument");
    float pairs[2 * UNC_NKMER];
    model_default_pairs(pairs);
    return model_make(pairs, "unc_model_default", out);
}

extern "C" int unc_model_from_pairs(const float *means_stdvs2048, unc_model_t **out) {
    if (!means_stdvs2048 || !out) return fail(UNC_ERR_ARG, "unc_model_from_pairs: null argument");
    *out = nullptr;
    return model_make(means_stdvs2048, "unc_model_from_pairs", out);
}

extern "C" void unc_model_free(unc_model_t *m) { delete m; }

static const char MODEL_BASES[] = "ACGT";
static const char MODEL_HEADER[] = "kmer\tlevel_mean\tlevel_stdv";

extern "C" int unc_model_load(const char *path, unc_model_t **out) {
    if (!path || !out) return fail(UNC_ERR_ARG, "unc_model_load: null argument");
    *out = nullptr;
    FILE *fp = fopen(path, "rb");
    if (!fp) return fail(UNC_ERR_IO, "unc_model_load: cannot read %s", path);
    std::string txt;
    char buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;) {
        txt.append(buf, got);
        if (txt.size() > (1u << 24)) break;     // (a model file is some 30 KB)
    }
    fclose(fp);
    if (txt.size() > (1u << 24)) return fail(UNC_ERR_ARG, "unc_model_load: %s is no model file (more than 16 MiB)", path);
    size_t at = txt.find('\n');                 // std::getline(model_in, _), pore_model.hpp:113
    at = at == std::string::npos ? txt.size() : at + 1;
    auto token = [&](std::string *t) {          // operator>> of a string: whitespace-separated
        while (at < txt.size() && isspace((unsigned char)txt[at])) ++at;
        const size_t st = at;
        while (at < txt.size() && !isspace((unsigned char)txt[at])) ++at;
        t->assign(txt, st, at - st);
        return at > st;
    };
    auto number = [&](const std::string &t, float *v) {
        if (t.empty()) return false;
        char *end = nullptr;
        *v = strtof(t.c_str(), &end);
        return end == t.c_str() + t.size() && std::isfinite(*v);
    };
    float pairs[2 * UNC_NKMER];
    std::vector<uint8_t> seen(UNC_NKMER, 0);
    std::string ks, ms, ss;
    for (uint32_t i = 0; i < (uint32_t)UNC_NKMER; ++i) {
        if (!token(&ks)) return fail(UNC_ERR_ARG, "unc_model_load: %s: ran out of k-mers after %u of %d", path, i, UNC_NKMER);
        if (!token(&ms) || !token(&ss)) return fail(UNC_ERR_ARG, "unc_model_load: %s: k-mer %s has no mean and stdv", path, ks.c_str());
        uint32_t kmer = 0;                      // str_to_kmer, bp.hpp:69-75
        bool ok = ks.size() == UNC_KLEN;
        for (size_t b = 0; ok && b < ks.size(); ++b) {
            const char *p = strchr(MODEL_BASES, ks[b]);
            if (!p || !ks[b]) ok = false;
            else kmer = (kmer << 2) | (uint32_t)(p - MODEL_BASES);
        }
        if (!ok) return fail(UNC_ERR_ARG, "unc_model_load: %s: k-mer '%s' is invalid", path, ks.c_str());
        if (seen[kmer]) return fail(UNC_ERR_ARG, "unc_model_load: %s: k-mer %s twice", path, ks.c_str());
        seen[kmer] = 1;
        float mean = 0, stdv = 0;
        if (!number(ms, &mean) || !number(ss, &stdv))
            return fail(UNC_ERR_ARG, "unc_model_load: %s: k-mer %s: '%s' '%s' are not two finite numbers", path, ks.c_str(), ms.c_str(), ss.c_str());
        if (!(stdv > 0)) return fail(UNC_ERR_ARG, "unc_model_load: %s: k-mer %s: stdv %g is not above 0", path, ks.c_str(), stdv);
        pairs[2 * kmer] = mean;
        pairs[2 * kmer + 1] = stdv;
    }
    // (1024 different k-mers of 1024: none is missing)
    if (token(&ks)) return fail(UNC_ERR_ARG, "unc_model_load: %s: '%s' behind the last of %d k-mers", path, ks.c_str(), UNC_NKMER);
    return model_make(pairs, "unc_model_load", out);
}

extern "C" int unc_model_save(const unc_model_t *m, const char *path) {
    if (!m || !path) return fail(UNC_ERR_ARG, "unc_model_save: null argument");
    FILE *fp = fopen(path, "wb");
    if (!fp) return fail(UNC_ERR_IO, "unc_model_save: cannot write %s", path);
    bool ok = fprintf(fp, "%s\n", MODEL_HEADER) > 0;
    for (uint32_t k = 0; k < (uint32_t)UNC_NKMER && ok; ++k) {
        char ks[UNC_KLEN + 1];
        for (int b = 0; b < UNC_KLEN; ++b) ks[b] = MODEL_BASES[(k >> (2 * (UNC_KLEN - 1 - b))) & 3];
        ks[UNC_KLEN] = 0;
        ok = fprintf(fp, "%s\t%.9g\t%.9g\n", ks, (double)m->pairs[2 * k], (double)m->pairs[2 * k + 1]) > 0;
    }
    ok = (fclose(fp) == 0) && ok;
    return ok ? UNC_OK : fail(UNC_ERR_IO, "unc_model_save: writing %s failed", path);
}

extern "C" int unc_model_pairs(const unc_model_t *m, float *out2048) {
    if (!m || !out2048) return fail(UNC_ERR_ARG, "unc_model_pairs: null argument");
    memcpy(out2048, m->pairs, sizeof m->pairs);
    return UNC_OK;
}

extern "C" int unc_model_tables(const unc_model_t *m, int cmpl, float *means1024, float *vars_x2_1024, float *lognorm1024, float *model_mean,
                                float *model_stdv) {
    if (!m) return fail(UNC_ERR_ARG, "unc_model_tables: null argument");
    ModelTables built;
    const ModelTables *t = &m->fwd;
    if (cmpl) { model_build_tables(m->pairs, true, &built); t = &built; }
    if (means1024) memcpy(means1024, t->tab, UNC_NKMER * 4);
    if (vars_x2_1024) memcpy(vars_x2_1024, t->tab + UNC_NKMER, UNC_NKMER * 4);
    if (lognorm1024) memcpy(lognorm1024, t->tab + 2 * UNC_NKMER, UNC_NKMER * 4);
    if (model_mean) *model_mean = t->mean;
    if (model_stdv) *model_stdv = t->stdv;
    return UNC_OK;
}
