// bg_objective_host_check.cpp -- a stand-alone program over the two *_host entries of include/burgers/objective.h, for a
// host sanitizer build (make -C csrc bg-objective-asan: AddressSanitizer + UBSan on the host code of bg_objective.hip,
// device code not instrumented).  Every buffer is a heap block of exactly the size the entry may touch, so a read or
// write past a row, an action table or the forcing matrix is reported; the shapes are those of
// tests/test_burgers_objective_host.py (every width of the stepper under both objectives, with and without actions; the
// row reward at each lane-group width's N, a ragged N and the smallest N, through a field, through actions and without
// forcing).  It makes no HIP call and needs no GPU.  Exit 0 and "ok" when every call returned what it should and every
// value written is finite.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/burgers/objective.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N, int E, int A) {
    if (!ok) {
        ++failures;
        std::fprintf(stderr, "FAILED %s at N=%d E=%d A=%d: %s\n", what, N, E, A, bg_objective_last_error());
    }
}

float noise(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f;
}

void run_step(int N, int E, int A, long n_substeps) {
    const float dx = 6.2831853f / (float)N, dt = N < 1024 ? 5e-4f : 1e-4f, nu = 0.02f;
    unsigned seed = 5u + (unsigned)(N + E + A);
    std::vector<float> u0((size_t)E * N), act((size_t)E * (A ? A : 1)), F((size_t)(A ? A : 1) * N);
    for (float& v : u0) v = noise(seed);
    for (float& v : act) v = noise(seed);
    for (float& v : F) v = noise(seed);
    std::vector<float> state[2];
    for (int objective = 0; objective < 2; ++objective) {
        std::vector<float> u = u0, obs((size_t)E * N);
        std::vector<double> sum(E);
        std::vector<int> status(E);
        expect(bg_step_objective_host(u.data(), A ? act.data() : nullptr, A ? F.data() : nullptr, A, E, N, dx, dt, nu,
                                      n_substeps, obs.data(), sum.data(), status.data(), objective) == 0,
               "bg_step_objective_host", N, E, A);
        for (int e = 0; e < E; ++e) expect(std::isfinite(sum[e]) && status[e] == 0, "a finite sum and a clear status", N, E, A);
        expect(obs == u, "obs = u", N, E, A);
        // the optional outputs may be absent
        std::vector<float> again = u0;
        expect(bg_step_objective_host(again.data(), A ? act.data() : nullptr, A ? F.data() : nullptr, A, E, N, dx, dt, nu,
                                      n_substeps, nullptr, nullptr, nullptr, objective) == 0, "no optional outputs", N, E, A);
        expect(again == u, "the same state without the optional outputs", N, E, A);
        state[objective] = u;
    }
    expect(state[0] == state[1], "the same state under both objectives", N, E, A);
    // the refusals read nothing
    expect(bg_step_objective_host(nullptr, nullptr, nullptr, 0, E, N, dx, dt, nu, 1, nullptr, nullptr, nullptr, 0) == -1,
           "a refusal", N, E, A);
    expect(bg_step_objective_host(u0.data(), nullptr, nullptr, 0, E, N, dx, dt, nu, 1, nullptr, nullptr, nullptr, 2) == -1,
           "a refusal", N, E, A);
    expect(bg_step_objective_host(u0.data(), nullptr, nullptr, 0, E, N + 1, dx, dt, nu, 1, nullptr, nullptr, nullptr, 1) == -4,
           "a refusal", N, E, A);
}

void run_rows(int N, int M, int A) {
    const double dx = 6.283185307179586 / N, nu = 0.01;
    unsigned seed = 17u + (unsigned)N;
    std::vector<float> u((size_t)M * N), phi((size_t)M * N), act((size_t)M * A), F((size_t)A * N);
    for (float& v : u) v = noise(seed);
    for (float& v : phi) v = noise(seed);
    for (float& v : act) v = noise(seed);
    for (float& v : F) v = noise(seed);
    std::vector<double> r(M);
    expect(bg_reward_rows_host(u.data(), phi.data(), nullptr, nullptr, M, N, 0, dx, nu, r.data()) == 0, "rows with a field", N, M, A);
    for (double v : r) expect(std::isfinite(v), "a finite reward", N, M, A);
    expect(bg_reward_rows_host(u.data(), nullptr, act.data(), F.data(), M, N, A, dx, nu, r.data()) == 0, "rows with actions", N, M, A);
    for (double v : r) expect(std::isfinite(v), "a finite reward", N, M, A);
    expect(bg_reward_rows_host(u.data(), nullptr, nullptr, nullptr, M, N, 0, dx, nu, r.data()) == 0, "rows without forcing", N, M, A);
    for (double v : r) expect(std::isfinite(v) && v <= 0.0, "a finite, non-positive reward", N, M, A);
    expect(bg_reward_rows_host(u.data(), phi.data(), act.data(), F.data(), M, N, A, dx, nu, r.data()) == -1, "a refusal", N, M, A);
    expect(bg_reward_rows_host(u.data(), nullptr, nullptr, nullptr, M, 2, 0, dx, nu, r.data()) == -1, "a refusal", N, M, A);
}

}  // namespace

int main() {
    const int widths[] = {64, 128, 256, 512, 1024};
    for (int N : widths) {
        run_step(N, 1, 0, 3);
        run_step(N, 5, 4, 3);
        run_step(N, 3, 16, N == 64 ? 50 : 2);
        run_step(N, 2, 1, 0);
    }
    const int rows[][3] = {{5, 2, 1}, {16, 3, 4}, {64, 3, 4}, {98, 5, 16}, {512, 2, 4}, {1024, 2, 4}, {3, 1, 1}};
    for (const auto& s : rows) run_rows(s[0], s[1], s[2]);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
