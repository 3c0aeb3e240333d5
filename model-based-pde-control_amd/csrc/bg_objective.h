// bg_objective.h -- the arithmetic of the Burgers objectives (include/burgers/objective.h): one lane's share of a midpoint
// sub-step with the reward term of either objective, and the row reward.  One spelling that bg_objective.hip compiles for
// the device (the kernels) and for the host (the *_host twins).  Nothing here is read by burgers.hip or bg_eval.hip.
// Built with -ffp-contract=off: every operation below is one rounded operation or one explicit fma.
//
// The step (bg_step_objective, bg_step_span_objective): the layout is bg_step_kernel's, lane = i / P owns the P
// contiguous points i = lane * P ... lane * P + P - 1 of an env's row, 64 lanes per env.  The state arithmetic is that
// kernel's, operation for operation (csrc/burgers.hip: the scalar form at P = 1, the pair form from P = 2, which at
// P = 2 is the packed window form with its one pair); the halo is handed in, so the device takes it from the neighbouring
// lanes by DPP and the host twin from the row.
//
// The order of the step's sum, which bg_step_objective_host reproduces bit for bit:
//   1. per lane and sub-step, at the state before the update, a chain over the lane's points in index order:
//        l2control    q  = fmaf(u_j, u_j, q)                                     term = (double)q
//        dissipation  qd = fmaf(g_j, g_j, qd),  qp = fmaf(u_j, phi_j, qp)        term = (double)qd * nu_d + (double)qp
//      with g_j the fp32 gradient of the stage-1 residual itself, (w[+1] - w[-1]) * half_inv_dx, and the dissipation
//      term formed by two separately rounded fp64 operations;
//   2. per lane, racc = racc + term over the sub-steps in order (the third fp64 operation);
//   3. across the 64 lanes, the xor butterfly m = 1, 2, 4, ..., 32: racc[l] = racc[l] + racc[l ^ m], a balanced tree.
//
// The row reward (bg_reward_rows): r = (-1.0) * (nu_d * (sum_i ux_i^2 / N) + sum_i u_i * phi_i / N) in fp64 from the
// widened fp32 values, ux = (u[+1] - u[-1]) / (2 dx) as bg_eval.h's `derivatives` forms it, nu_d = (double)(float)nu.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define BGO_HD __host__ __device__ inline
#else
#define BGO_HD inline
#endif

namespace bgo {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int L2CONTROL = 0, DISSIPATION = 1;   // BG_OBJECTIVE_*
constexpr int LANES = 64;

// the stencil coefficients of burgers.hip's set_coefficients, pre-divided once on the host, and the fp64 viscosity
struct Coef {
    float half_inv_dx;        // 1 / (2 dx)
    float l0, l1, l2;         // nu * laplace coefficients / dx^2: centre, +-1, +-2
    float dt, hdt;
    double nu_d;
};

inline Coef coefficients(float dx, float dt, float nu) {
    Coef c;
    c.half_inv_dx = 0.5f / dx;
    const float s = nu / (dx * dx);
    c.l0 = s * (-5.0f / 2.0f); c.l1 = s * (4.0f / 3.0f); c.l2 = s * (-1.0f / 12.0f);
    c.dt = dt; c.hdt = 0.5f * dt;
    c.nu_d = (double)nu;
    return c;
}

// phi = act @ F at column i: one rounded product, then one fmaf per further actuator, in index order
BGO_HD float forcing_at(const float* act, const float* F, int n_act, int N, int i) {
    float acc = act[0] * F[i];
    for (int k = 1; k < n_act; ++k) acc = fmaf(act[k], F[(size_t)k * N + i], acc);
    return acc;
}

// residual r = nu u_xx - u u_x + phi of a lane's P points v; lo = the two points left of its first (lo[1] the nearer),
// hi = the two right of its last (hi[0] the nearer).  With SUMS the dissipation chains qd, qp advance over the P points.
template <int P, bool SUMS>
BGO_HD void lane_residual(const float (&v)[P], const float (&lo)[2], const float (&hi)[2], const float (&phi)[P],
                          const Coef& c, float (&r)[P], float& qd, float& qp) {
    if constexpr (P == 1) {
        const float grad = (hi[0] - lo[1]) * c.half_inv_dx;
        float lap = fmaf(c.l0, v[0], phi[0]);
        lap = fmaf(c.l1, lo[1] + hi[0], lap);
        lap = fmaf(c.l2, lo[0] + hi[1], lap);
        r[0] = fmaf(-v[0], grad, lap);
        if constexpr (SUMS) {
            qd = fmaf(grad, grad, qd);
            qp = fmaf(v[0], phi[0], qp);
        }
    } else {
        // E[k] the aligned pairs of the window, O[k] = (E[k].hi, E[k+1].lo) the pairs at odd offsets
        constexpr int H = P / 2;
        f32x2 E[H + 2], O[H + 1];
        E[0] = f32x2{lo[0], lo[1]};
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k < H; ++k) E[k + 1] = f32x2{v[2 * k], v[2 * k + 1]};
        E[H + 1] = f32x2{hi[0], hi[1]};
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k <= H; ++k) O[k] = __builtin_shufflevector(E[k], E[k + 1], 1, 2);
        const f32x2 hid = {c.half_inv_dx, c.half_inv_dx}, l0 = {c.l0, c.l0}, l1 = {c.l1, c.l1}, l2 = {c.l2, c.l2};
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k < H; ++k) {
            // points 2k, 2k + 1: centre E[k+1], +-2 E[k] / E[k+2], -1 O[k], +1 O[k+1]
            const f32x2 ph = {phi[2 * k], phi[2 * k + 1]};
            const f32x2 grad = (O[k + 1] - O[k]) * hid;
            f32x2 lap = __builtin_elementwise_fma(l0, E[k + 1], ph);
            lap = __builtin_elementwise_fma(l1, O[k] + O[k + 1], lap);
            lap = __builtin_elementwise_fma(l2, E[k] + E[k + 2], lap);
            const f32x2 rr = __builtin_elementwise_fma(-E[k + 1], grad, lap);
            r[2 * k] = rr[0];
            r[2 * k + 1] = rr[1];
            if constexpr (SUMS) {
                qd = fmaf(grad[0], grad[0], qd);
                qd = fmaf(grad[1], grad[1], qd);
                qp = fmaf(v[2 * k], phi[2 * k], qp);
                qp = fmaf(v[2 * k + 1], phi[2 * k + 1], qp);
            }
        }
    }
}

// out = fmaf(a, r, u) at the lane's P points
template <int P>
BGO_HD void lane_axpy(float a, const float (&r)[P], const float (&u)[P], float (&out)[P]) {
    if constexpr (P == 1) {
        out[0] = fmaf(a, r[0], u[0]);
    } else {
        const f32x2 a2 = {a, a};
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k < P / 2; ++k) {
            const f32x2 o = __builtin_elementwise_fma(a2, f32x2{r[2 * k], r[2 * k + 1]}, f32x2{u[2 * k], u[2 * k + 1]});
            out[2 * k] = o[0];
            out[2 * k + 1] = o[1];
        }
    }
}

// the l2control chain of a lane: sum of squares of its P points in index order
template <int P>
BGO_HD float lane_ssq(const float (&u)[P]) {
    float q = 0.0f;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = 0; j < P; ++j) q = fmaf(u[j], u[j], q);
    return q;
}

// racc = racc + ((double)qd * nu_d + (double)qp): three separately rounded fp64 operations
BGO_HD void add_dissipation(double& racc, float qd, float qp, double nu_d) {
    const double d = (double)qd * nu_d;
    const double t = d + (double)qp;
    racc = racc + t;
}

// stage 1 of a sub-step: ut = u + dt/2 residual(u), and the sub-step's reward term into racc
template <int P, int OBJ>
BGO_HD void lane_stage1(const float (&u)[P], const float (&lo)[2], const float (&hi)[2], const float (&phi)[P],
                        const Coef& c, float (&ut)[P], double& racc) {
    float r[P], qd = 0.0f, qp = 0.0f;
    if constexpr (OBJ == L2CONTROL) racc += (double)lane_ssq<P>(u);
    lane_residual<P, OBJ == DISSIPATION>(u, lo, hi, phi, c, r, qd, qp);
    if constexpr (OBJ == DISSIPATION) add_dissipation(racc, qd, qp, c.nu_d);
    lane_axpy<P>(c.hdt, r, u, ut);
}

// stage 2: u = u + dt residual(ut); lo, hi the halo of ut
template <int P>
BGO_HD void lane_stage2(float (&u)[P], const float (&ut)[P], const float (&lo)[2], const float (&hi)[2],
                        const float (&phi)[P], const Coef& c) {
    float r[P], qd = 0.0f, qp = 0.0f;
    lane_residual<P, false>(ut, lo, hi, phi, c, r, qd, qp);
    lane_axpy<P>(c.dt, r, u, u);
}

// ---------------------------------------------------------------------------------------------------------------------
// the row reward
struct RewardArgs {
    const float* u;           // [M][N]
    const float* phi;         // [M][N] or null
    const float* actions;     // [M][A] or null (then F [A][N])
    const float* F;
    int M, N, A;
    double two_dx, nu_d;
    double* reward;           // [M]
};

BGO_HD int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// the share (first, first + step, ...) of row `row`: sd += ux^2, sp += u * phi
BGO_HD void reward_row_share(const RewardArgs& a, long row, int first, int step, double& sd, double& sp) {
    const float* r = a.u + row * a.N;
    for (int i = first; i < a.N; i += step) {
        const double ux = ((double)r[wrap(i + 1, a.N)] - (double)r[wrap(i - 1, a.N)]) / a.two_dx;
        sd += ux * ux;
        float p = 0.0f;
        if (a.phi) p = a.phi[row * a.N + i];
        else if (a.actions) p = forcing_at(a.actions + row * a.A, a.F, a.A, a.N, i);
        sp += (double)r[i] * (double)p;
    }
}

BGO_HD double reward_row_finish(double sd, double sp, int N, double nu_d) {
    return (-1.0) * (nu_d * (sd / N) + sp / N);
}

}  // namespace bgo
