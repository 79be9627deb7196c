#include "report.h"
#include <cstdio>

static double ratio(double num, double den) { return den > 0 ? num / den : 0.0; }

int gcn_class_report(int C, const int64_t *confusion, const int64_t *tp, const int64_t *fp, const int64_t *fn, ClassReport *out,
                     std::string *err) {
    auto fail = [&](const std::string &why) {
        if (err) *err = "class_report: " + why;
        return -1;
    };
    if (!out) return fail("no output");
    if (C < 1) return fail("the number of classes must be at least 1");
    const bool vectors = tp || fp || fn;
    if (vectors && !(tp && fp && fn)) return fail("tp, fp and fn go together");
    if (vectors == (confusion != nullptr)) return fail("give either a confusion matrix or tp / fp / fn");
    ClassReport r;
    r.tp.assign(C, 0); r.fp.assign(C, 0); r.fn.assign(C, 0);
    if (confusion) {
        std::vector<int64_t> row(C, 0), col(C, 0);
        for (int t = 0; t < C; t++)
            for (int p = 0; p < C; p++) {
                const int64_t v = confusion[(size_t)t * C + p];
                if (v < 0) return fail("negative count at (" + std::to_string(t) + ", " + std::to_string(p) + ")");
                row[t] += v; col[p] += v; r.rows += v;
            }
        for (int c = 0; c < C; c++) {
            r.tp[c] = confusion[(size_t)c * C + c];
            r.fp[c] = col[c] - r.tp[c];
            r.fn[c] = row[c] - r.tp[c];
        }
    } else {
        for (int c = 0; c < C; c++) {
            if (tp[c] < 0 || fp[c] < 0 || fn[c] < 0) return fail("negative count for class " + std::to_string(c));
            r.tp[c] = tp[c]; r.fp[c] = fp[c]; r.fn[c] = fn[c];
        }
    }
    r.support.resize(C); r.precision.resize(C); r.recall.resize(C); r.f1.resize(C);
    double sum_f1 = 0, TP = 0, FP = 0, FN = 0;
    for (int c = 0; c < C; c++) {
        const double a = (double)r.tp[c], b = (double)r.fp[c], d = (double)r.fn[c];
        r.support[c] = a + d;
        r.precision[c] = ratio(a, a + b);
        r.recall[c] = ratio(a, a + d);
        r.f1[c] = ratio(2 * a, 2 * a + b + d);
        sum_f1 += r.f1[c];
        TP += a; FP += b; FN += d;
    }
    r.macro_f1 = sum_f1 / C;
    r.micro_f1 = ratio(2 * TP, 2 * TP + FP + FN);
    r.accuracy = confusion ? ratio(TP, (double)r.rows) : 0.0;
    *out = std::move(r);
    return 0;
}

int gcn_class_report_write(const char *path, int C, const ClassReport &rep, const int64_t *confusion, std::string *err) {
    FILE *f = fopen(path, "w");
    bool ok = f != nullptr;
    for (int c = 0; ok && c < C; c++)
        ok = fprintf(f, "class %d support %lld precision %.6f recall %.6f f1 %.6f\n", c, (long long)rep.support[c], rep.precision[c],
                     rep.recall[c], rep.f1[c]) > 0;
    if (ok) ok = fprintf(f, "macro_f1 %.6f micro_f1 %.6f\n", rep.macro_f1, rep.micro_f1) > 0;
    if (ok && confusion) {
        ok = fprintf(f, "confusion\n") > 0;
        for (int t = 0; ok && t < C; t++)
            for (int p = 0; ok && p < C; p++)
                ok = fprintf(f, p + 1 < C ? "%lld " : "%lld\n", (long long)confusion[(size_t)t * C + p]) > 0;
    }
    if (f && fclose(f) != 0) ok = false;
    if (!ok && err) *err = std::string("could not write the report to ") + path;
    return ok ? 0 : -1;
}
