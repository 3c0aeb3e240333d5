/*
 * burgers_oracle.c -- fp32 twin of the viscous-Burgers stepper's arithmetic.  TEST INFRASTRUCTURE ONLY.
 *
 * Written from include/burgers_hip.h and the order of operations below, not from the kernels: flat loops over the
 * grid index, neighbours by (i + k + N) % N, no lanes, no pairs, no windows.  Every operation is one separately
 * rounded fp32 operation or one fmaf (correctly rounded: libm's or the hardware instruction); the file must be built
 * with -ffp-contract=off (oracle/Makefile) so that the compiler fuses nothing else.
 *
 *   coefficients (all fp32, from fp32 dx, dt, nu):
 *     hid = 0.5f / dx      s = nu / (dx * dx)      l0 = s * (-5.0f / 2.0f)   l1 = s * (4.0f / 3.0f)
 *     l2  = s * (-1.0f / 12.0f)                    hdt = 0.5f * dt
 *   forcing:   phi[i] = act[0] * F[0][i];  phi[i] = fmaf(act[k], F[k][i], phi[i]) for k = 1 .. n_act-1;  no actions: 0
 *   residual:  grad = (u[i+1] - u[i-1]) * hid
 *              lap  = fmaf(l0, u[i], phi[i]);  lap = fmaf(l1, u[i-1] + u[i+1], lap);  lap = fmaf(l2, u[i-2] + u[i+2], lap)
 *              r[i] = fmaf(-u[i], grad, lap)
 *   sub-step:  ut = fmaf(hdt, r(u), u);  u = fmaf(dt, r(ut), u)
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    float hid, l0, l1, l2, dt, hdt;
} coef_t;

static coef_t coefficients(float dx, float dt, float nu) {
    coef_t c;
    const float s = nu / (dx * dx);
    c.hid = 0.5f / dx;
    c.l0 = s * (-5.0f / 2.0f);
    c.l1 = s * (4.0f / 3.0f);
    c.l2 = s * (-1.0f / 12.0f);
    c.dt = dt;
    c.hdt = 0.5f * dt;
    return c;
}

/* r = residual of one row; phi may be NULL (then 0) */
static void residual_row(const float* u, const float* phi, int N, const coef_t* c, float* r) {
    for (int i = 0; i < N; ++i) {
        const float um2 = u[(i - 2 + N) % N], um1 = u[(i - 1 + N) % N], u0 = u[i];
        const float up1 = u[(i + 1 + N) % N], up2 = u[(i + 2 + N) % N];
        const float grad = (up1 - um1) * c->hid;
        float lap = fmaf(c->l0, u0, phi ? phi[i] : 0.0f);
        lap = fmaf(c->l1, um1 + up1, lap);
        lap = fmaf(c->l2, um2 + up2, lap);
        r[i] = fmaf(-u0, grad, lap);
    }
}

/* out [n_rows, N] = residual(u [n_rows, N]) (+ phi [n_rows, N] unless NULL); any N >= 5 */
int bgo_residual(const float* u, const float* phi, int n_rows, int N, float dx, float nu, float* out) {
    if (!u || !out || n_rows <= 0 || N < 5 || !(dx > 0.0f)) return -1;
    const coef_t c = coefficients(dx, 1.0f, nu);
    for (int e = 0; e < n_rows; ++e)
        residual_row(u + (size_t)e * N, phi ? phi + (size_t)e * N : NULL, N, &c, out + (size_t)e * N);
    return 0;
}

/* u [E, N] in/out advanced by n_substeps midpoint sub-steps; actions [E, n_act] with F [n_act, N], or actions NULL for
 * no forcing; ssq [E] (or NULL) = sum over sub-steps of sum_i u_i^2 of the fp32 state BEFORE each update, in fp64;
 * before [E, n_substeps, N] (or NULL) = the state before each sub-step. */
int bgo_step_states(float* u, const float* actions, const float* F, int n_act, int E, int N, float dx, float dt, float nu,
                    long n_substeps, double* ssq, float* before) {
    if (!u || E <= 0 || N < 5 || n_substeps < 0 || !(dx > 0.0f)) return -1;
    if (actions && (!F || n_act <= 0)) return -1;
    const coef_t c = coefficients(dx, dt, nu);
    float* buf = (float*)malloc(sizeof(float) * 3 * (size_t)N);
    if (!buf) return -2;
    float *phi = buf, *r = buf + N, *ut = buf + 2 * (size_t)N;
    for (int e = 0; e < E; ++e) {
        float* row = u + (size_t)e * N;
        for (int i = 0; i < N; ++i) {
            float acc = 0.0f;
            if (actions) {
                const float* act = actions + (size_t)e * n_act;
                acc = act[0] * F[i];
                for (int k = 1; k < n_act; ++k) acc = fmaf(act[k], F[(size_t)k * N + i], acc);
            }
            phi[i] = acc;
        }
        double total = 0.0;
        for (long s = 0; s < n_substeps; ++s) {
            if (before) memcpy(before + ((size_t)e * n_substeps + s) * N, row, sizeof(float) * N);
            double q = 0.0;
            for (int i = 0; i < N; ++i) q += (double)row[i] * (double)row[i];
            total += q;
            residual_row(row, phi, N, &c, r);
            for (int i = 0; i < N; ++i) ut[i] = fmaf(c.hdt, r[i], row[i]);
            residual_row(ut, phi, N, &c, r);
            for (int i = 0; i < N; ++i) row[i] = fmaf(c.dt, r[i], row[i]);
        }
        if (ssq) ssq[e] = total;
    }
    free(buf);
    return 0;
}

int bgo_step(float* u, const float* actions, const float* F, int n_act, int E, int N, float dx, float dt, float nu,
             long n_substeps, double* ssq) {
    return bgo_step_states(u, actions, F, n_act, E, N, dx, dt, nu, n_substeps, ssq, NULL);
}
