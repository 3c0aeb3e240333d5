// Internal (non-ABI) declarations shared by ks_kernels.hip, ks_capi.hip and ks_cpu.cpp: the step constants and the KS
// arithmetic that the fused kernels, the LDS kernel and the CPU twin all run (one spelling, two compilers), and the
// launch declarations (hipcc only).  ks_cpu.cpp includes this under a plain C++ compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <type_traits>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KS_HD __host__ __device__ __forceinline__
#else
#define KS_HD inline
#endif

namespace ks {

// The constants of one (dx, dt): formed once on the host (make_consts), read by every kernel and by the twin.
struct Consts {
    // fast mode
    double c_lin[5];       // merged linear stencil: -(D4_k/dx^4 + D2_k/dx^2), k = 0..4
    double mh_inv_dx;      // -0.5 / dx
    double hdt, dt6, dt3;  // dt/2, dt/6, dt/3
    // both modes
    double dt;
    // exact mode: the reference's divisors and their correctly rounded reciprocals (div_const)
    double dx, dx2, dx4;
    double r_dx, r_dx2, r_dx4;   // (also the fast-mode dissipation scale factors of the sel^2 / lap^2 sums)
};

inline Consts make_consts(double dx, double dt) {
    Consts c;
    c.dt = dt;
    c.dx = dx;
    c.dx2 = dx * dx;            // python: self.dx**2
    c.dx4 = std::pow(dx, 4.0);  // python: self.dx**4
    c.r_dx = 1.0 / c.dx;        // IEEE divisions on the host: correctly rounded reciprocals
    c.r_dx2 = 1.0 / c.dx2;
    c.r_dx4 = 1.0 / c.dx4;
    // merged linear stencil  -(u_xxxx + u_xx):  c_k = -(D4_k/dx^4 + D2_k/dx^2)
    const double d2[5] = {-49.0 / 18, 3.0 / 2, -3.0 / 20, 1.0 / 90, 0.0};
    const double d4[5] = {91.0 / 8, -122.0 / 15, 169.0 / 60, -2.0 / 5, 7.0 / 240};
    for (int k = 0; k < 5; ++k) c.c_lin[k] = -(d4[k] / c.dx4 + d2[k] / c.dx2);
    c.mh_inv_dx = -0.5 / dx;
    c.hdt = dt / 2.0;
    c.dt6 = dt / 6.0;
    c.dt3 = dt / 3.0;
    return c;
}

// Everything a fused-stepper launch needs; passed by value (lands in SGPRs).
struct StepArgs {
    double* u;             // [E,N] fp64 state, in/out
    const float* phi;      // [E,N] fp32 forcing field or nullptr
    const float* actions;  // [E,n_act] fp32 or nullptr
    const float* F;        // [n_act,N] fp32 forcing matrix (needed iff actions)
    const int* env_ids;    // [n_rows] subset or nullptr (identity)
    float* obs;            // [E,N] fp32 out or nullptr (indexed by env id)
    double* ssq_sum;       // [E] out or nullptr (indexed by env id)
    int* status;           // [E] out or nullptr (indexed by env id)
    int n_rows;            // number of envs this launch processes
    int n_act;
    int N;
    long n_substeps;
    Consts k;              // the step constants (make_consts); last, so that the offsets of the members above stay put
};

// f(EXACT, DISS) with the two run-time flags as std::bool_constant arguments: the one place where (mode, objective)
// become template arguments, for the kernel launches and for the twin.
template <class F>
inline auto with_flags(bool exact, bool diss, F&& f) {
    if (exact) return diss ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return diss ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// x / d for a divisor d that is constant over the launch, bit-identical to the IEEE division the reference performs:
//   q = RN(x * r),  e = x - d * q (exact in one FMA),  result = RN(q + e * r),   r = RN(1 / d) from the host
// (Markstein's correction step: with a correctly rounded reciprocal one step from the faithful q lands on the correctly
// rounded quotient).  3 VALU instructions instead of the ~11 of the generic fp64 division sequence (v_div_scale x 2, v_rcp,
// 5 FMA, v_div_fmas, v_div_fixup) -- the exact mode spends 17 divisions per point and sub-step, 47 % of its instructions.
// Checked bit for bit against x / d on 7e9 dividends incl. ones placed next to rounding boundaries
// (tools/micro/markstein_check.c) and, end to end, by the golden tests (200 000-sub-step reset, bit-identical state).
// Not covered: x = -0.0 (gives +0.0; unreachable -- every dividend here is a sum whose coefficients have both signs, so a
// vanishing sum is +0.0) and non-finite x (the env raises FloatingPointError on those anyway).
KS_HD double div_const(double x, double d, double r) {
    const double q = x * r;
    const double e = __builtin_fma(-d, q, x);
    return __builtin_fma(e, r, q);
}

// Division policies of the reference-order arithmetic.  The stepper kernels and the reward kernel divide by div_const;
// the rhs test hook and the twin keep the true division.  The golden tests pin both forms to the same bits: that is
// the end-to-end check of div_const.
struct DivMarkstein {
    static KS_HD double div(double x, double d, double r) { return div_const(x, d, r); }
};
struct DivIeee {
    static KS_HD double div(double x, double d, double) { return x / d; }
};

// ------------------------------------------------------------------------------------------
// rhs at one grid point.  w[] is a window of u with 4 halo values on both sides of the points, q[] = w[]^2, c the index
// of the point inside the window.
// ------------------------------------------------------------------------------------------
// Reference operation order.  ref_terms: the reference's u_x (d1, upwind derivative of u^2) and u_xx (d2), all the
// dissipation reward reads; it takes its two divisors and their reciprocals as scalars, so a caller without a whole
// Consts (ks_reward_rows_kernel) passes exactly what is read.  ref_point: these two, u_xxxx (d4) and the rhs.
struct RefTerms {
    double d1, d2;
};
template <class DIV>
KS_HD RefTerms ref_terms(const double* w, const double* q, int c, double dx, double r_dx, double dx2, double r_dx2) {
    // scipy correlate1d summation order (ni_filters.c walks the flipped kernel from the far right tap): see
    // oracle/ks_oracle.c
    double fwd = q[c + 4] * (-1.0 / 4);
    fwd += q[c] * (-25.0 / 12);
    fwd += q[c + 1] * 4.0;
    fwd += q[c + 2] * (-3.0);
    fwd += q[c + 3] * (4.0 / 3);
    double bwd = q[c - 4] * (1.0 / 4);
    bwd += q[c - 3] * (-4.0 / 3);
    bwd += q[c - 2] * 3.0;
    bwd += q[c - 1] * (-4.0);
    bwd += q[c] * (25.0 / 12);
    const double f = DIV::div(fwd, dx, r_dx), b = DIV::div(bwd, dx, r_dx);
    const double u = w[c];
    RefTerms t;
    t.d1 = (u < 0.0 ? 1.0 : 0.0) * f + (u >= 0.0 ? 1.0 : 0.0) * b;   // u == 0 -> backward
    double d2 = u * (-49.0 / 18);
    d2 += (w[c - 3] + w[c + 3]) * (1.0 / 90);
    d2 += (w[c - 2] + w[c + 2]) * (-3.0 / 20);
    d2 += (w[c - 1] + w[c + 1]) * (3.0 / 2);
    t.d2 = DIV::div(d2, dx2, r_dx2);
    return t;
}
struct RefPoint {
    double d1, d2, d4, rhs;
};
template <class DIV>
KS_HD RefPoint ref_point(const double* w, const double* q, int c, double phi, const Consts& a) {
    const RefTerms t = ref_terms<DIV>(w, q, c, a.dx, a.r_dx, a.dx2, a.r_dx2);
    const double u = w[c];
    RefPoint p;
    p.d1 = t.d1;
    p.d2 = t.d2;
    double d4 = u * (91.0 / 8);
    d4 += (w[c - 4] + w[c + 4]) * (7.0 / 240);
    d4 += (w[c - 3] + w[c + 3]) * (-2.0 / 5);
    d4 += (w[c - 2] + w[c + 2]) * (169.0 / 60);
    d4 += (w[c - 1] + w[c + 1]) * (-122.0 / 15);
    p.d4 = DIV::div(d4, a.dx4, a.r_dx4);
    p.rhs = ((-p.d4 - p.d2) - 0.5 * p.d1) + phi;
    return p;
}

// Fast mode: merged linear stencil + both upwind sums sharing the centre term, every accumulator's FMA chain in the
// order of rhs_tile_fast and rhs_hybrid_fast (ks_kernels.hip), so all fast-mode forms give the same bits.
// TERMS (dissipation objective): also the two reward terms unscaled -- sel, the selected upwind sum (= u_x * dx up to
// sign), and lap, the 7-point u_xx stencil (= u_xx * dx^2); the caller scales their sums once per launch.
struct FastPoint {
    double k, sel, lap;
};
template <bool TERMS>
KS_HD FastPoint fast_point(const double* w, const double* q, int c, double phi, const Consts& a) {
    FastPoint p;
    p.lap = 0.0;
    if constexpr (TERMS) {
        double lap = (-49.0 / 18) * w[c];
        lap = __builtin_fma(3.0 / 2, w[c - 1] + w[c + 1], lap);
        lap = __builtin_fma(-3.0 / 20, w[c - 2] + w[c + 2], lap);
        p.lap = __builtin_fma(1.0 / 90, w[c - 3] + w[c + 3], lap);
    }
    double lin = __builtin_fma(a.c_lin[0], w[c], phi);
    lin = __builtin_fma(a.c_lin[1], w[c - 1] + w[c + 1], lin);
    lin = __builtin_fma(a.c_lin[2], w[c - 2] + w[c + 2], lin);
    lin = __builtin_fma(a.c_lin[3], w[c - 3] + w[c + 3], lin);
    lin = __builtin_fma(a.c_lin[4], w[c - 4] + w[c + 4], lin);
    // backward upwind table b = (25/12, -4, 3, -4/3, 1/4); forward table is its negation
    double bw = (25.0 / 12) * q[c];
    double fw = __builtin_fma(4.0, q[c + 1], -bw);   // fw holds MINUS the forward sum
    bw = __builtin_fma(-4.0, q[c - 1], bw);
    fw = __builtin_fma(-3.0, q[c + 2], fw);
    bw = __builtin_fma(3.0, q[c - 2], bw);
    fw = __builtin_fma(4.0 / 3, q[c + 3], fw);
    bw = __builtin_fma(-4.0 / 3, q[c - 3], bw);
    fw = __builtin_fma(-0.25, q[c + 4], fw);
    bw = __builtin_fma(0.25, q[c - 4], bw);
    p.sel = (w[c] < 0.0) ? fw : bw;                  // u == 0 selects the backward stencil
    p.k = __builtin_fma(a.mh_inv_dx, p.sel, lin);
    return p;
}

// Classical RK4, stage STAGE = 1..4 at one point: k is the rhs of the stage, u the state at the start of the
// sub-step, acc the running weighted sum.  Stages 1..3 write acc and the next stage's state usn; stage 4 reads acc and
// writes the new state to usn.  EXACT keeps the reference's order (kuramoto.py:86-90; DIV as in ref_point), FAST uses
// pre-divided steps and FMAs with u folded into acc.
template <bool EXACT, int STAGE, class DIV = DivMarkstein>
KS_HD void rk4_update(double k, double u, double& acc, double& usn, const Consts& a) {
    static_assert(STAGE >= 1 && STAGE <= 4, "RK4 has four stages");
    if constexpr (EXACT) {
        if constexpr (STAGE == 1) acc = k;
        if constexpr (STAGE == 2 || STAGE == 3) acc = acc + 2.0 * k;
        if constexpr (STAGE <= 2) usn = u + a.dt * k / 2.0;
        if constexpr (STAGE == 3) usn = u + a.dt * k;
        if constexpr (STAGE == 4) usn = u + DIV::div(a.dt * (acc + k), 6.0, 1.0 / 6.0);
    } else {
        if constexpr (STAGE == 1) acc = __builtin_fma(a.dt6, k, u);
        if constexpr (STAGE == 2 || STAGE == 3) acc = __builtin_fma(a.dt3, k, acc);
        if constexpr (STAGE <= 2) usn = __builtin_fma(a.hdt, k, u);
        if constexpr (STAGE == 3) usn = __builtin_fma(a.dt, k, u);
        if constexpr (STAGE == 4) usn = __builtin_fma(a.dt6, k, acc);
    }
}

struct Layout {
    int variant;       // ks_variant
    int G;             // lanes per env (0 for LDS variant)
    int P;             // points per lane
    int block;         // threads per workgroup
    int grid;          // workgroups
    size_t lds_bytes;  // dynamic LDS
};

#ifdef __HIPCC__
// Returns false if (variant, N) has no instantiated kernel.
bool layout_supported(int variant, int N);
// Launch the fused stepper described by `lay` on `stream`.  objective (ks_objective) selects what a.ssq_sum
// accumulates; without a reward buffer the l2control kernels run.  The hybrid layouts have no dissipation form
// (hipErrorNotSupported).
hipError_t launch_step(const Layout& lay, int mode, int objective, const StepArgs& a, hipStream_t stream);
// per-row reward of fp32 obs [n,N] with fp32 phi [n,N] (phi may be null) -> fp64 out [n] (device pointers)
hipError_t launch_reward_rows(int objective, const float* obs, const float* phi, int n_rows, int N, double dx,
                              double* out, hipStream_t stream);
// ks_record_device: transition w = t * E + e of a segment goes to replay row dst[w] (device pointers; `scale` is
// -1.0 * (1.0 / N), formed on the host)
struct RecordArgs {
    const float* traj;      // [T + 1][E][N]
    const float* actions;   // [T][E][A]
    const double* ssq;      // [T][E]
    const int* steps;       // [T][E]
    const long* dst;        // [T][E]
    float* obs;
    float* act;
    float* nxtobs;
    float* rewards;
    unsigned char* terminated;
    unsigned char* truncated;
    int* out_steps;
    long rows, n;           // slab rows; T * E
    int E, N, A;
    int vec_obs, vec_act;
    double scale, substeps;
};
hipError_t launch_record(const RecordArgs& a, hipStream_t stream);
// rhs test hook: u [n,N], phi [n,N] -> outputs [n,N] (device pointers; ux/uxx/uxxxx may be null)
hipError_t launch_rhs(const double* u, const float* phi, int n_rows, int N, double dx, double dx2,
                      double dx4, double* rhs, double* ux, double* uxx, double* uxxxx,
                      hipStream_t stream);
// cross-lane primitive self-test; d_fail is a device unsigned (bit per ks_variant)
hipError_t launch_selftest(unsigned* d_fail, hipStream_t stream);
#endif  // __HIPCC__

}  // namespace ks
