// ks_cpu.cpp -- CPU twin of the fused KS stepper (see ks_cpu.h).  Compiled with -ffp-contract=off: the exact mode must keep
// the reference's unfused multiply / add order; the fast mode spells its FMAs out.  The per-point arithmetic and the RK4
// stage updates are the ones of ks_internal.h, the text the GPU kernels are built from; the twin keeps the true division.
//
// What is computed (reference, paths relative to the reference root):
//   pdegym/kuramoto/kuramoto.py:118-129  rhs(u, phi) with the periodic stencil tables :24-27
//   pdegym/kuramoto/kuramoto.py:83-90    per sub-step: reward term (before the update), then classical RK4
//   pdegym/common/transforms.py:262-265  phi = action @ F in fp32
// One env is advanced through all its sub-steps by one thread on a window padded by the +-4 periodic halo, so the
// stencil loops carry no index arithmetic and vectorise; envs are spread over host threads (they never interact).
#include "ks_cpu.h"

#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <vector>

namespace kscpu {
namespace {

struct Scratch {
    std::vector<double> w, q, k, acc, us, phi, t1, t2;
    explicit Scratch(int N) : w(N + 8), q(N + 8), k(N), acc(N), us(N), phi(N), t1(N), t2(N) {}
};

// w[4 + i] = x[i], halo of 4 on both sides wrapped periodically; q = w * w
inline void window(const double* x, int N, double* w, double* q) {
    for (int i = 0; i < N; ++i) w[4 + i] = x[i];
    for (int m = 0; m < 4; ++m) {
        w[m] = x[N - 4 + m];
        w[N + 4 + m] = x[m];
    }
    for (int i = 0; i < N + 8; ++i) q[i] = w[i] * w[i];
}

// reference operation order with true divisions (ks::ref_point, kuramoto.py:118-129) over a padded row
inline void rhs_exact(const Consts& c, const double* w, const double* q, const double* phi, int N, double* out, double* ux,
                      double* uxx, double* uxxxx) {
    for (int i = 0; i < N; ++i) {
        const ks::RefPoint p = ks::ref_point<ks::DivIeee>(w, q, i + 4, phi[i], c);
        out[i] = p.rhs;
        if (ux) ux[i] = p.d1;
        if (uxx) uxx[i] = p.d2;
        if (uxxxx) uxxxx[i] = p.d4;
    }
}

// k = rhs of one stage over a padded row.  TERMS (stage 1 of the dissipation objective): also the per-point reward terms
// t1 / t2 -- EXACT the reference's u_x and u_xx, FAST the unscaled sel and lap of ks::fast_point.
template <bool EXACT, bool TERMS>
inline void rhs_row(const Consts& c, const double* w, const double* q, const double* phi, int N, double* k, double* t1,
                    double* t2) {
    if constexpr (EXACT) {
        rhs_exact(c, w, q, phi, N, k, TERMS ? t1 : nullptr, TERMS ? t2 : nullptr, nullptr);
    } else {
        for (int i = 0; i < N; ++i) {
            const ks::FastPoint p = ks::fast_point<TERMS>(w, q, i + 4, phi[i], c);
            k[i] = p.k;
            if constexpr (TERMS) {
                t1[i] = p.sel;
                t2[i] = p.lap;
            }
        }
    }
}

// DISS: the reward accumulator collects the dissipation terms (kspde.h ks_objective) instead of sum u^2
template <bool EXACT, bool DISS>
void advance_env(int N, const Consts& c, double* u, const double* phi, long n_substeps, Scratch& s, double* ssq_out) {
    double* w = s.w.data();
    double* q = s.q.data();
    double* k = s.k.data();
    double* acc = s.acc.data();
    double* us = s.us.data();
    double* t1 = s.t1.data();
    double* t2 = s.t2.data();
    // one RK4 stage: the rhs at the stage state (stage 1's is formed with the reward terms, below), then the stage's
    // update (ks::rk4_update; stage 4 writes the new u)
    auto stage = [&](auto stage_no) {
        constexpr int STAGE = decltype(stage_no)::value;
        if constexpr (STAGE > 1) {
            window(us, N, w, q);
            rhs_row<EXACT, false>(c, w, q, phi, N, k, nullptr, nullptr);
        }
        double* next = STAGE == 4 ? u : us;
        for (int i = 0; i < N; ++i) ks::rk4_update<EXACT, STAGE, ks::DivIeee>(k[i], u[i], acc[i], next[i], c);
    };
    double racc = 0.0;
    double rx = 0.0, rxx = 0.0;   // fast-mode dissipation: unscaled sel^2 / lap^2 sums
    for (long step = 0; step < n_substeps; ++step) {
        // stage 1 + the reward term of this sub-step (taken BEFORE the update, kuramoto.py:84)
        window(u, N, w, q);
        rhs_row<EXACT, DISS>(c, w, q, phi, N, k, t1, t2);
        if constexpr (!DISS) {
            double row = 0.0;
            for (int i = 0; i < N; ++i) row += q[4 + i];
            racc += row;
        } else if constexpr (EXACT) {
            double row = 0.0;
            for (int i = 0; i < N; ++i) row += (t2[i] * t2[i] + t1[i] * t1[i]) + w[4 + i] * phi[i];
            racc += row;
        } else {
            for (int i = 0; i < N; ++i) {
                racc = __builtin_fma(w[4 + i], phi[i], racc);
                rx = __builtin_fma(t1[i], t1[i], rx);
                rxx = __builtin_fma(t2[i], t2[i], rxx);
            }
        }
        stage(std::integral_constant<int, 1>{});
        stage(std::integral_constant<int, 2>{});
        stage(std::integral_constant<int, 3>{});
        stage(std::integral_constant<int, 4>{});
    }
    if constexpr (DISS && !EXACT) racc = __builtin_fma(rxx, c.r_dx4, __builtin_fma(rx, c.r_dx2, racc));
    *ssq_out = racc;
}

void run_rows(int N, const Consts& c, int mode, int objective, double* u, const float* phi, const float* actions, const float* F,
              int n_act, const int* env_ids, int lo, int hi, long n_substeps, float* obs, double* ssq_sum, int* status) {
    Scratch s(N);
    for (int r = lo; r < hi; ++r) {
        const int env = env_ids ? env_ids[r] : r;
        double* ue = u + (size_t)env * N;
        if (phi) {
            for (int i = 0; i < N; ++i) s.phi[i] = (double)phi[(size_t)env * N + i];
        } else if (actions) {
            // fp32 FMA chain in action-index order == torch's CPU matmul (transforms.py:264)
            const float* act = actions + (size_t)env * n_act;
            for (int i = 0; i < N; ++i) {
                float a = act[0] * F[i];
                for (int k = 1; k < n_act; ++k) a = __builtin_fmaf(act[k], F[(size_t)k * N + i], a);
                s.phi[i] = (double)a;
            }
        } else {
            std::fill(s.phi.begin(), s.phi.end(), 0.0);
        }
        double ssq = 0.0;
        // without a reward buffer the objective is irrelevant (the GPU runs its l2control kernels then, too)
        const bool diss = objective == 1 && ssq_sum;
        ks::with_flags(mode == 1, diss, [&](auto exact, auto dissipation) {
            advance_env<decltype(exact)::value, decltype(dissipation)::value>(N, c, ue, s.phi.data(), n_substeps, s, &ssq);
        });
        int bad = 0;
        for (int i = 0; i < N; ++i) bad |= !std::isfinite(ue[i]);
        if (obs)
            for (int i = 0; i < N; ++i) obs[(size_t)env * N + i] = (float)ue[i];
        if (ssq_sum) ssq_sum[env] = ssq;
        if (status) status[env] = bad;
    }
}

}  // namespace

int default_threads() {
    int n = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::max(1, CPU_COUNT(&set));
    if (const char* e = std::getenv("KSPDE_CPU_THREADS")) {
        const int v = std::atoi(e);
        if (v > 0) n = std::min(n, v);
    }
    return n;
}

void step(int N, const Consts& c, int mode, int objective, double* u, const float* phi, const float* actions, const float* F,
          int n_act, const int* env_ids, int n_rows, long n_substeps, float* obs, double* ssq_sum, int* status, int n_threads) {
    if (n_rows <= 0) return;
    // a thread is worth starting for >= ~1e6 point-sub-steps of its own
    const double work = (double)n_rows * (double)N * (double)std::max<long>(n_substeps, 1);
    int T = std::max(1, std::min({n_threads, n_rows, (int)(work / 1e6) + 1}));
    if (T == 1) {
        run_rows(N, c, mode, objective, u, phi, actions, F, n_act, env_ids, 0, n_rows, n_substeps, obs, ssq_sum, status);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(T - 1);
    const int per = n_rows / T, extra = n_rows % T;
    int lo = 0;
    for (int t = 0; t < T; ++t) {
        const int hi = lo + per + (t < extra ? 1 : 0);
        if (t + 1 < T)
            pool.emplace_back(run_rows, N, std::cref(c), mode, objective, u, phi, actions, F, n_act, env_ids, lo, hi,
                              n_substeps, obs, ssq_sum, status);
        else
            run_rows(N, c, mode, objective, u, phi, actions, F, n_act, env_ids, lo, hi, n_substeps, obs, ssq_sum, status);
        lo = hi;
    }
    for (auto& th : pool) th.join();
}

void rhs(int N, const Consts& c, const double* u, const float* phi, int n_rows, double* out, double* ux, double* uxx,
         double* uxxxx) {
    Scratch s(N);
    for (int r = 0; r < n_rows; ++r) {
        const size_t off = (size_t)r * N;
        for (int i = 0; i < N; ++i) s.phi[i] = (double)phi[off + i];
        window(u + off, N, s.w.data(), s.q.data());
        rhs_exact(c, s.w.data(), s.q.data(), s.phi.data(), N, out + off, ux ? ux + off : nullptr,
                  uxx ? uxx + off : nullptr, uxxxx ? uxxxx + off : nullptr);
    }
}

void reward_rows(int N, const Consts& c, int objective, const float* obs, const float* phi, int n_rows, double* out) {
    Scratch s(N);
    std::vector<double> uu(N), rhs(N), zero(N, 0.0);
    for (int r = 0; r < n_rows; ++r) {
        const size_t off = (size_t)r * N;
        for (int i = 0; i < N; ++i) uu[i] = (double)obs[off + i];
        double sxx = 0.0, sx = 0.0, sup = 0.0;
        if (objective == 1) {
            window(uu.data(), N, s.w.data(), s.q.data());
            rhs_exact(c, s.w.data(), s.q.data(), zero.data(), N, rhs.data(), s.t1.data(), s.t2.data(), nullptr);
            for (int i = 0; i < N; ++i) {
                sxx += s.t2[i] * s.t2[i];
                sx += s.t1[i] * s.t1[i];
                if (phi) sup += uu[i] * (double)phi[off + i];
            }
            out[r] = (-1.0) * ((sxx / N + sx / N) + sup / N);
        } else {
            for (int i = 0; i < N; ++i) sup += uu[i] * uu[i];
            out[r] = (-1.0) * (1.0 / N) * sup;
        }
    }
}

void record(int E, int N, int A, long n, const float* traj, const float* actions, const double* ssq, const int* steps,
            const long* dst, double scale, double substeps, float* obs, float* act, float* nxtobs, float* rewards,
            unsigned char* terminated, unsigned char* truncated, int* out_steps) {
    for (long w = 0; w < n; ++w) {
        const long r = dst[w];
        if (r < 0) continue;
        std::memcpy(obs + r * N, traj + w * N, sizeof(float) * N);
        std::memcpy(nxtobs + r * N, traj + (w + E) * N, sizeof(float) * N);
        std::memcpy(act + r * A, actions + w * A, sizeof(float) * A);
        rewards[r] = (float)((scale * ssq[w]) / substeps);
        out_steps[r] = steps[w];
        terminated[r] = truncated[r] = 0;
    }
}

void eval_rows(int objective, const ks::EvalArgs& a) {
    ks::with_flags(true, objective == 1, [&](auto, auto dissipation) {
        constexpr bool DISS = decltype(dissipation)::value;
        for (long row = 0; row < (long)a.B * a.T; ++row) {
            ks::EvalSums sums = {};
            ks::eval_row_share<ks::DivIeee, DISS>(a, row, 0, 1, sums);
            ks::eval_row_finish<DISS>(sums, a.N, a.rowstats + row * ks::EVAL_ROW_STATS);
        }
    });
}

void eval_fold(const double* rowstats, int B, int T, int N, double* tables, double* accum) {
    for (int i = 0; i < 1 + ks::EVAL_TABLES * T; ++i) {
        tables[i] = ks::eval_fold_value(rowstats, B, T, N, i);
        if (accum) accum[i] += (double)B * tables[i];
    }
}

}  // namespace kscpu
