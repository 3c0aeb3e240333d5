// bg_eval_host_check.cpp -- a stand-alone program over the three *_host entries of include/burgers/eval.h, for a host
// sanitizer build (make -C csrc bg-eval-asan: AddressSanitizer + UBSan on the host code of bg_eval.hip, device code not
// instrumented).  Every buffer is a heap block of exactly the size the entry may touch, so a read or write past a row, a
// table or a coefficient array is reported; the shapes are those of tests/_bg_eval_oracle.py (each lane-group width's N, a
// ragged N, the smallest N), through each inverse kind, batch- and time-major predictions, with and without the shift, the
// outputs and the accumulator.  It makes no HIP call and needs no GPU.  Exit 0 and "ok" when every call returned 0 and
// every value written is finite.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/burgers/eval.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N, int B, int T) {
    if (!ok) {
        ++failures;
        std::fprintf(stderr, "FAILED %s at N=%d B=%d T=%d: %s\n", what, N, B, T, bg_eval_last_error());
    }
}

float noise(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f;
}

void run(int N, int B, int T) {
    const double dx = 6.283185307179586 / N;
    unsigned seed = 17u + (unsigned)N;
    std::vector<float> truth((size_t)B * T * N), pred((size_t)B * T * N), coef4((size_t)4 * N), coef2((size_t)2 * N);
    for (float& v : truth) v = noise(seed);
    for (size_t i = 0; i < pred.size(); ++i) pred[i] = truth[i] * 1.03f + 0.01f * noise(seed);
    for (int i = 0; i < N; ++i) {
        coef4[i] = -1.25f; coef4[N + i] = 2.5f; coef4[2 * N + i] = 5.0f; coef4[3 * N + i] = -2.5f;
        coef2[i] = 1.5f; coef2[N + i] = 0.25f;
    }
    const int S = BG_EVAL_ROW_STATS, n_tables = 1 + BG_EVAL_TABLES * T;
    for (int kind = 0; kind <= 2; ++kind) {
        for (int layout = 0; layout < 2; ++layout) {       // 0: batch-major prediction, no shift; 1: time-major, shifted
            std::vector<float> t_out((size_t)B * T * N), p_out((size_t)B * T * N);
            std::vector<double> stats((size_t)B * T * S), tables(n_tables), accum(n_tables, 0.0);
            bg_eval_batch in{};
            in.truth = truth.data(); in.truth_bstride = (long)T * N; in.truth_tstride = N;
            in.pred = pred.data();
            in.pred_bstride = layout ? N : (long)T * N;
            in.pred_tstride = layout ? (long)B * N : N;
            in.pred_shift = layout;
            in.inv_kind = kind; in.inv_coef = kind == 1 ? coef4.data() : kind == 2 ? coef2.data() : nullptr;
            in.truth_out = layout ? t_out.data() : nullptr; in.pred_out = layout ? p_out.data() : nullptr;
            expect(bg_eval_rows_host(&in, B, T, N, dx, stats.data()) == 0, "bg_eval_rows_host", N, B, T);
            for (double v : stats) expect(std::isfinite(v), "a finite row statistic", N, B, T);
            expect(bg_eval_fold_host(stats.data(), B, T, N, tables.data(), accum.data()) == 0, "bg_eval_fold_host", N, B, T);
            expect(bg_eval_fold_host(stats.data(), B, T, N, tables.data(), nullptr) == 0, "bg_eval_fold_host", N, B, T);
            for (int i = 0; i < n_tables; ++i) expect(accum[i] == (double)B * tables[i], "accum = B * tables", N, B, T);
        }
    }
    std::vector<double> ux((size_t)B * T * N), uxx((size_t)B * T * N);
    expect(bg_derivatives_host(truth.data(), B * T, N, dx, ux.data(), uxx.data()) == 0, "bg_derivatives_host", N, B, T);
    for (size_t i = 0; i < ux.size(); ++i) expect(std::isfinite(ux[i]) && std::isfinite(uxx[i]), "a finite derivative", N, B, T);
    // the refusals read nothing
    expect(bg_eval_rows_host(nullptr, B, T, N, dx, nullptr) == -1, "a refusal", N, B, T);
    expect(bg_derivatives_host(truth.data(), B * T, 4, dx, ux.data(), uxx.data()) == -1, "a refusal", N, B, T);
}

}  // namespace

int main() {
    const int shapes[][3] = {{64, 3, 7}, {100, 3, 7}, {256, 2, 5}, {1024, 2, 3}, {48, 17, 1}, {5, 2, 2}};
    for (const auto& s : shapes) run(s[0], s[1], s[2]);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
